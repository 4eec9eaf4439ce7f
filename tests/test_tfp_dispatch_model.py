"""The host-side model of dspsr_amd_tfp_filterbank's launch arithmetic (tests/tfp_cases.py) and the case table that
tests/test_gpu_tfp.py builds from it: for every device size the table must make workgroups of all four kernel families walk
several items -- the cross-item prefetch, the "more tiles follow" predicate, the restart of the running sums and the hand-over
of the LDS image are not executed otherwise.  Runs without a GPU."""
import pytest

import tfp_cases as tc


def test_model_restates_the_counts_of_known_launches():
    # the largest launch of tests/test_gpu_parity.py: 18 items, one per workgroup
    d = tc.dispatch(512, 16, 300, False, 0, 256)
    assert (d.family, d.T, d.groups_per_out, d.nout, d.nitem, d.grid) == (tc.K_TFPM, 16, 1, 18, 18, 18)
    # the benchmark: 32768 parts of 4096 channels, tscrunch 16 -- 2048 items of 8 tiles, eight items per workgroup
    d = tc.dispatch(4096, 16, 32768, False, 0, 256)
    assert (d.family, d.T, d.groups_per_out, d.nitem, d.grid) == (tc.K_TFP4K, 2, 8, 2048, 256)
    # tscrunch below the tile: items are tiles, the last one may be partly filled; tscrunch 0 means 1
    d = tc.dispatch(64, 4, 1000, True, 0, 256)
    assert (d.family, d.T, d.groups_per_out, d.nout, d.nitem) == (tc.K_TFP_COAL, 128, 1, 250, 8)
    assert tc.dispatch(64, 0, 1000, True, 8, 256) == tc.dispatch(64, 1, 1000, True, 8, 256)
    assert tc.dispatch(64, 0, 1000, True, 8, 256)[:5] == (tc.K_TFP_HALF, 128, 1, 1000, 8)
    # an unaligned block never takes a register-split kernel; 8192 channels (T = 1) aligned always does
    assert tc.dispatch(4096, 16, 64, False, 2, 256).family == tc.K_TFP_HALF
    assert tc.dispatch(1024, 8, 64, True, 8, 256).family == tc.K_TFP_HALF
    assert all(tc.dispatch(8192, sf, 64, False, 0, 256).family == tc.K_TFPM for sf in (1, 2, 3, 5, 16))
    assert tc.dispatch(4096, 1, 64, False, 0, 256).family == tc.K_TFP_COAL
    assert tc.dispatch(2048, 2, 64, False, 0, 256).family == tc.K_TFP_COAL and tc.dispatch(2048, 4, 64, False, 0, 256).family == tc.K_TFPM
    # nothing to do / refused
    d = tc.dispatch(4096, 16, 15, False, 0, 256)
    assert d.family is None and d.refused is None and d.grid == 0
    for args, text in (((8, 1, 64, False, 0, 256), "must be a power of two"), ((16384, 1, 64, False, 0, 256), "must be a power of two"),
                       ((48, 1, 64, False, 0, 256), "must be a power of two"), ((4096, 3, 64, False, 0, 256), "must divide or be a multiple of 2 parts"),
                       ((512, 24, 64, False, 0, 256), "must divide or be a multiple of 16 parts"),
                       ((64, 1, 64, False, 1, 256), "2-byte aligned"), ((64, 1, 64, True, 3, 256), "2-byte aligned")):
        d = tc.dispatch(*args)
        assert d.family is None and text in d.refused, args
    assert "npol=1" in tc.dispatch(64, 1, 64, False, 0, 256, npol=1).refused


@pytest.mark.parametrize("ncu", [64, 256, 304, 7])
def test_case_table_gives_every_family_several_items_per_workgroup(ncu):
    by_family = {f: [] for f in tc.FAMILIES}
    for c in tc.all_cases(ncu):
        d = tc.dispatch(c.nchan, c.tscrunch, c.npart, c.caspsr, c.align, ncu)
        assert d.refused is None and d.family is not None, c
        by_family[d.family].append((c, d))
    several = lambda d: d.nitem >= 2 * ncu + 1 and d.grid == ncu
    for family, lst in by_family.items():
        # some workgroups take three items, the others two
        assert any(several(d) and d.nitem % ncu != 0 and d.nitem < 3 * ncu for _c, d in lst), family
        # an output sample of several tiles, several output samples per workgroup
        assert any(d.groups_per_out > 1 and several(d) for _c, d in lst), family
        # the parts behind the last whole output sample are not written
        assert any(c.npart % c.tscrunch and several(d) for c, d in lst), family
        # both byte orders, with and without the polarisation sum
        assert {(c.caspsr, c.pscrunch) for c, _d in lst} == {(False, False), (False, True), (True, False), (True, True)}, family
        if family in (tc.K_TFP_COAL, tc.K_TFP_HALF):
            # output samples end inside a tile
            assert any(1 < c.tscrunch < d.T and several(d) for c, d in lst), family
            assert any(c.tscrunch == 1 and d.T > 1 and several(d) for c, d in lst), family
    # the anchor: the half-word kernel at tscrunch 1 for every channel count and both byte orders, blocks of at most 64 MB
    for c in tc.anchor_cases(ncu):
        d = tc.dispatch(c.nchan, c.tscrunch, c.npart, c.caspsr, c.align, ncu)
        assert d.family == tc.K_TFP_HALF and c.tscrunch == 1 and d.nitem >= tc.items_wanted(ncu) >= 2 * ncu + ncu // 2 + 1
        assert c.npart * 4 * c.nchan <= 64 << 20 or ncu > 256
    assert {(c.nchan, c.caspsr) for c in tc.anchor_cases(ncu)} == {(n, o) for n in tc.ALL_NCHAN for o in (False, True)}
    assert len({c.pscrunch for c in tc.anchor_cases(ncu)}) == 2
    # the exact cases fall into the family they are listed under
    ex = [(c, tc.dispatch(c.nchan, c.tscrunch, c.npart, c.caspsr, c.align, ncu)) for c in tc.exact_cases(ncu)]
    assert all(several(d) for _c, d in ex)
    fours = {c.tscrunch for c, d in ex if d.family == tc.K_TFP4K}
    assert {2, 16} <= fours and any(sf & (sf - 1) for sf in fours)
    for nchan in (512, 1024, 2048, 8192):
        sfs = {c.tscrunch for c, d in ex if d.family == tc.K_TFPM and c.nchan == nchan}
        assert 8192 // nchan in sfs and any(sf > 8192 // nchan for sf in sfs), nchan
    assert any(c.nchan == 8192 and c.tscrunch % 2 and c.tscrunch > 1 for c, d in ex if d.family == tc.K_TFPM)
    for nchan in (512, 1024, 2048, 4096, 8192):           # every instantiation of the register-split kernels
        assert len({(c.caspsr, c.pscrunch) for c, d in ex if d.family in (tc.K_TFPM, tc.K_TFP4K) and c.nchan == nchan}) == 4, nchan
    coal = [(c, d) for c, d in ex if d.family == tc.K_TFP_COAL]
    assert {c.nchan for c, _d in coal} == set(tc.ALL_NCHAN) - {8192}            # (8192 aligned: k_tfpm for every factor)
    for nchan in tc.ALL_NCHAN:
        rel = {(c.tscrunch > d.T) - (c.tscrunch < d.T) for c, d in coal if c.nchan == nchan}
        assert rel == ({-1, 0, 1} if nchan < 512 else {-1} if nchan <= 4096 else set()), nchan
    assert any(c.nchan == 4096 and c.tscrunch == 1 for c, _d in coal)
    # the benchmark's geometry: eight items per workgroup; the CASPSR offsets 2, 4, 8: the half-word kernel
    b = tc.bench_case(ncu)
    d = tc.dispatch(b.nchan, b.tscrunch, b.npart, b.caspsr, b.align, ncu)
    assert (d.family, d.groups_per_out, d.nitem) == (tc.K_TFP4K, 8, 8 * ncu)
    offs = tc.caspsr_offset_cases(ncu)
    assert {c.align for c in offs} == {2, 4, 8} and all(c.caspsr for c in offs)
    assert all(tc.dispatch(c.nchan, c.tscrunch, c.npart, True, c.align, ncu).family == tc.K_TFP_HALF for c in offs)
    assert {tc.dispatch(c.nchan, c.tscrunch, c.npart, True, 0, ncu).family for c in offs} == {tc.K_TFP4K, tc.K_TFPM, tc.K_TFP_COAL}
    nchan, sf, ppb = tc.chain_case(ncu)
    assert ppb % sf == 0 and tc.dispatch(nchan, sf, ppb, False, 0, ncu).nout > 2 * ncu
    # ids are unique: one pytest case each
    ids = [tc.case_id(c) for c in tc.exact_cases(ncu)]
    assert len(set(ids)) == len(ids)


def test_npart_for_gives_the_items_asked_for():
    for nchan in tc.ALL_NCHAN:
        T = 8192 // nchan
        for sf in (1, 2, 3, 4, 6, 16, T, 2 * T, 3 * T, max(1, T // 4)):
            if sf % T and T % sf:
                continue
            for nitem in (1, 2, 161, 641):
                for ragged in (False, True):
                    npart = tc.npart_for(nchan, sf, nitem, ragged)
                    d = tc.dispatch(nchan, sf, npart, False, 0, 64)
                    assert d.nitem == nitem and (npart % sf != 0) == (ragged and sf > 1), (nchan, sf, nitem, ragged)
                    if sf < T:
                        assert (d.nout * sf) % T == sf % T                # the last tile holds one output sample
