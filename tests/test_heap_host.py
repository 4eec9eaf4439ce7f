"""MeerKAT heaps (INSTRUMENT MKBF / MKBFRo) on the host side: the numpy reorders of dspsr_amd.dada against the loop restatement of
tests/heap_cases.py, DadaFile on synthetic files (ndat from whole heaps, blocks of whole heaps with the first sample's place in
them, the per-channel slices, the header refusals), the block sizes of the drivers, the plan-time refusals of the drivers that have
no heap reader, and the constants of the binding.  No device."""
from types import SimpleNamespace

import numpy as np
import pytest

import heap_cases as hc


@pytest.mark.parametrize("machine", sorted(hc.MACHINES))
@pytest.mark.parametrize("npol", [1, 2])
@pytest.mark.parametrize("nchan", [1, 3, 64])
def test_reorders_match_the_restatement(machine, npol, nchan):
    from dspsr_amd import dada
    swap = hc.MACHINES[machine]
    rng = np.random.default_rng(nchan * 10 + npol)
    tfp = rng.integers(-128, 128, (3 * hc.HEAP, nchan, npol, 2), dtype=np.int8)
    heaps = dada.heaps_from_tfp(tfp, swap)
    assert heaps.dtype == np.int8 and heaps.size == tfp.size
    want = hc.heaps_from_stream(np.ascontiguousarray(tfp.transpose(1, 2, 0, 3)), swap)
    assert np.array_equal(heaps.reshape(-1), want)
    stream = hc.stream_from_heaps(heaps, nchan, npol, swap)                     # [nchan][npol][ndat][2]
    assert np.array_equal(stream.transpose(2, 0, 1, 3), tfp)
    back = dada.tfp_from_heaps(heaps, nchan, npol, swap)
    assert back.shape == tfp.shape and np.array_equal(back, tfp)
    if nchan * npol > 1 or swap:
        assert not np.array_equal(heaps.reshape(-1), tfp.reshape(-1))          # (the heap order is not the TFP order)
    with pytest.raises(Exception, match="multiple of 256"):
        dada.heaps_from_tfp(tfp[:300], swap)
    with pytest.raises(Exception, match="whole heaps"):
        dada.tfp_from_heaps(heaps.reshape(-1)[:-2], nchan, npol, swap)


def test_lib_constants_and_raw_at():
    from dspsr_amd import _lib
    import dspsr_amd
    assert (_lib.RAW_MEERKAT, _lib.RAW_MEERKAT_SWAP) == (3, 4) == (dspsr_amd.RAW_MEERKAT, dspsr_amd.RAW_MEERKAT_SWAP)
    assert _lib.raw_at(_lib.RAW_MEERKAT, 0) == 3 and _lib.raw_at(_lib.RAW_MEERKAT_SWAP, 0) == 4
    assert _lib.raw_at(_lib.RAW_MEERKAT, 1) == 3 | (1 << 8) and _lib.raw_at(_lib.RAW_MEERKAT_SWAP, 255) == 4 | (255 << 8)
    assert dspsr_amd.raw_at is _lib.raw_at
    for layout, first in ((_lib.RAW_GENERIC, 1), (_lib.RAW_CASPSR, 0), (_lib.RAW_UWB16, 3), (_lib.RAW_MEERKAT, 256), (_lib.RAW_MEERKAT, -1)):
        with pytest.raises(ValueError):
            _lib.raw_at(layout, first)
    assert _lib.is_heaps(_lib.raw_at(_lib.RAW_MEERKAT_SWAP, 200)) and _lib.is_heaps(3) and not _lib.is_heaps(_lib.RAW_UWB16)
    assert not _lib.is_heaps(256) and not _lib.is_heaps(-1)
    # the header's macros say the same
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dspsr_amd.h")).read()
    assert re.search(r"#define DSPSR_AMD_RAW_MEERKAT\s+3\b", text) and re.search(r"#define DSPSR_AMD_RAW_MEERKAT_SWAP\s+4\b", text)
    assert re.search(r"#define DSPSR_AMD_RAW_AT\(layout, first_sample\)\s+\(\(layout\) \| \(\(first_sample\) << 8\)\)", text)
    for name in ("dspsr_amd_unpack_heaps_fpt", "dspsr_amd_filterbank_takes_heaps"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)


def _stand_in(ppb, step, ovl, form):
    return SimpleNamespace(cfg=SimpleNamespace(parts_per_block=ppb), nsamp_step=step, nsamp_overlap=ovl, form=form)


@pytest.mark.parametrize("machine", sorted(hc.MACHINES))
@pytest.mark.parametrize("nchan,npol", [(1, 2), (3, 1), (4, 2)])
def test_dada_file_of_heaps(tmp_path, machine, nchan, npol):
    from dspsr_amd import dada
    swap = hc.MACHINES[machine]
    nheap = 9
    block = hc.random_block(nheap, nchan, npol, seed=5)
    # (a trailing partial heap is not data: ndat counts whole heaps)
    path = hc.write_dada(tmp_path / "a.dada", np.concatenate([block, np.zeros(100, np.int8)]), machine=machine, nchan=nchan, npol=npol)
    f = dada.DadaFile(path)
    assert f.heaps and f.info.machine == machine and f.ndat == nheap * hc.HEAP
    ppb, step, ovl = 2, 301, 211                                # odd step: blocks start at many places inside a heap
    lt = _stand_in(ppb, step, ovl, f.form)
    assert (f.form.name, f.form.granule) == ("heaps", hc.HEAP)
    full, rest = f.nblocks(lt)
    assert (full, rest) == divmod((f.ndat - ovl) // step, ppb) and full >= 3
    stream = hc.stream_from_heaps(block, nchan, npol, swap)
    per_heap = hc.heap_bytes(1, nchan, npol)
    got = list(f.blocks(lt))
    assert len(got) == full + (1 if rest else 0)
    firsts = []
    for b, (view, npart, first) in enumerate(got):
        s0 = b * ppb * step
        assert npart == (ppb if b < full else rest)
        assert first == s0 & 255
        firsts.append(first)
        nsamp = npart * step + ovl
        assert view.size % per_heap == 0 and view.size == hc.heap_bytes(-(-(first + nsamp) // 256), nchan, npol)     # whole heaps
        assert np.array_equal(view, block[(s0 >> 8) * per_heap:(s0 >> 8) * per_heap + view.size])
        # the samples of the block, read back through the restatement, are the stream's
        mine = hc.stream_from_heaps(view, nchan, npol, swap)[:, :, first:first + nsamp]
        assert np.array_equal(mine, stream[:, :, s0:s0 + nsamp])
    assert any(firsts[1:]), "the case must start a later block inside a heap"
    # channel slices: a block of heaps with nchan = 1
    for g in range(nchan):
        for b, (view, npart, first) in enumerate(f.blocks(lt, channel=g)):
            s0 = b * ppb * step
            nsamp = npart * step + ovl
            assert first == s0 & 255 and view.size == hc.heap_bytes(-(-(first + nsamp) // 256), 1, npol)
            mine = hc.stream_from_heaps(view, 1, npol, swap)[:, :, first:first + nsamp]
            assert np.array_equal(mine[0], stream[g, :, s0:s0 + nsamp])


def test_dada_file_header_refusals(tmp_path):
    from dspsr_amd import DspsrAmdError, dada
    block = hc.random_block(2, 2, 2)
    with pytest.raises(DspsrAmdError, match="NDIM"):
        dada.DadaFile(hc.write_dada(tmp_path / "ndim.dada", block, machine="MKBF", nchan=2, npol=2, ndim=1))
    with pytest.raises(DspsrAmdError, match="NBIT"):
        dada.DadaFile(hc.write_dada(tmp_path / "nbit.dada", block, machine="MKBFRo", nchan=2, npol=2, nbit=16))
    with pytest.raises(DspsrAmdError, match="NPOL"):
        dada.DadaFile(hc.write_dada(tmp_path / "npol.dada", block, machine="MKBF", nchan=1, npol=4))
    # the generic reader is as it was: the same bytes under INSTRUMENT DADA are TFP samples
    f = dada.DadaFile(hc.write_dada(tmp_path / "tfp.dada", block, machine="DADA", nchan=2, npol=2))
    assert not f.heaps and f.ndat == block.size // 8
    view, npart, first = next(iter(f.blocks(_stand_in(1, 100, 20, f.form))))
    assert npart == 1 and view.size == 120 * 8 and first == 0 and f.form.name == "generic"


def test_block_bytes_of_the_drivers():
    from dspsr_amd import _lib, inputs, pipeline
    machine_layout = lambda machine: inputs.raw_form(pipeline.InputInfo(machine=machine)).layout
    for machine, layout in (("MKBF", _lib.RAW_MEERKAT), ("MKBFRo", _lib.RAW_MEERKAT_SWAP)):
        assert machine_layout(machine) == layout
    assert machine_layout("CASPSR") == _lib.RAW_CASPSR and machine_layout("DADA") == _lib.RAW_GENERIC
    info = pipeline.InputInfo(nchan=4, npol=2, ndim=2, machine="MKBF")
    drv = SimpleNamespace(cfg=SimpleNamespace(parts_per_block=3), nsamp_step=301, nsamp_overlap=211, layout=_lib.RAW_MEERKAT, in_nchan=4,
                          info=info, form=inputs.raw_form(info))
    for cls in (pipeline.LoadToFold, pipeline.ConvolvingFront):             # (LoadToFilCoherent's and LoadToFITS's blocks with -F)
        for npart, first in ((None, 0), (3, 0), (1, 0), (2, 255), (3, 17), (1, 1)):
            nsamp = (npart or 3) * 301 + 211
            assert cls.block_bytes(drv, npart, first) == hc.heap_bytes(-(-(first + nsamp) // 256), 4, 2)
            assert drv.form.block_bytes(nsamp, 4, 2, 2, first) == cls.block_bytes(drv, npart, first)
            # (a layout word that already carries a first sample sizes the same block)
            drv.layout = _lib.raw_at(_lib.RAW_MEERKAT, 9)
            assert cls.block_bytes(drv, npart, first) == hc.heap_bytes(-(-(first + nsamp) // 256), 4, 2)
            drv.layout = _lib.RAW_MEERKAT
    # the other layouts size their blocks as before, and take no first sample
    drv.layout, drv.form = _lib.RAW_GENERIC, inputs.raw_form(pipeline.InputInfo(nchan=4, npol=2, ndim=2, machine="DADA"))
    assert pipeline.LoadToFold.block_bytes(drv, 2) == (2 * 301 + 211) * 4 * 2 * 2
    with pytest.raises(Exception, match="first_sample"):
        pipeline.LoadToFold.block_bytes(drv, 2, 5)


def test_drivers_without_a_heap_reader_refuse_by_name():
    from dspsr_amd import DspsrAmdError, pipeline
    for machine in sorted(hc.MACHINES):
        info = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=-16.0, nchan=4, npol=2, ndim=2, tsamp_us=0.25, machine=machine)
        with pytest.raises(DspsrAmdError, match="LoadToFilDirect.*INSTRUMENT %s" % machine):
            pipeline.LoadToFilDirect(pipeline.SearchConfig(nchan=4, tscrunch=1, nbit=8, parts_per_block=1024), info)
        with pytest.raises(DspsrAmdError, match="LoadToFil:.*INSTRUMENT %s" % machine):
            pipeline.LoadToFil(pipeline.SearchConfig(nchan=64, tscrunch=1, nbit=8, parts_per_block=16), info)
        one = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=-4.0, nchan=1, npol=2, ndim=2, tsamp_us=0.25, machine=machine)
        cfg = pipeline.Config(nchan=1, dispersion_measure=10.0, nbin=64, folding_period=0.004, freq_res=1024, zap_rfi=True)
        with pytest.raises(DspsrAmdError, match=r"-R.*INSTRUMENT %s" % machine):
            pipeline.LoadToFold(cfg, one)
