"""The kernels of the square-law fold (dspsr -d 1, -d 2) in the SHIPPED library, read from its AMDGPU metadata as
tests/test_kernel_resources.py reads the others: the fused inverse pass k_inv_chan<., 3 | 7, .> of every transform length the
host can pick, the stand-alone fold's instantiations for rows of ndim 1 and the scalar combine of the partial profiles exist;
the forms with a compile-time tile (the ones fb_pick_kernels takes for a full 2^14-point tile: the headline's among them) use no
scratch and at most 256 VGPRs.  CPU only: nothing is launched."""
import pytest

from test_kernel_resources import kernels          # noqa: F401  (the fixture)

FULL_LOGT = {logf: 14 - logf for logf in range(0, 14)}            # fb_common.h full_logt
HEADLINE = ["k_inv_chan<12, 3, 2>", "k_inv_chan<12, 7, 2>"]
FOLD = ["k_fold_chunked<1, false, 1>", "k_fold_chunked<1, true, 1>", "k_fold_dense<1, 1>", "k_fold_many<1, 1>", "k_fold_direct<1>", "k_fold_combine"]
# spills of run-time-tile forms (LOGT = -1: tiles smaller than 2^14 points, geometries of few channels), bytes per lane.  Their
# Coherence twins k_inv_chan<., 1 | 5, -1> spill likewise at these lengths; none is launched by a BASELINE workload.
TOLERATED = {
    "k_inv_chan<12, 3, -1>": 64, "k_inv_chan<12, 7, -1>": 64, "k_inv_chan<13, 3, -1>": 72, "k_inv_chan<13, 7, -1>": 72,
    "k_inv_chan<10, 7, -1>": 8, "k_inv_chan<9, 7, -1>": 8,
}


def test_square_law_fold_kernels_exist(kernels):
    for logf in range(0, 14):
        for epip in (3, 7):
            for logt in (-1, FULL_LOGT[logf]):
                assert "k_inv_chan<%d, %d, %d>" % (logf, epip, logt) in kernels
    for name in FOLD:
        assert name in kernels, name


def test_square_law_fold_kernels_use_no_scratch(kernels):
    names = [n for n in kernels if n.startswith("k_inv_chan<") and n.split(",")[1].strip() in ("3", "7")]
    assert len(names) == 56
    for name in names + FOLD:
        kd = kernels[name]
        scratch = int(kd.get(".private_segment_fixed_size", 0))
        assert scratch <= TOLERATED.get(name, 0), "%s uses %d bytes of scratch per lane (%d VGPRs)" % (name, scratch, kd.get(".vgpr_count", -1))
        assert int(kd.get(".vgpr_count", 0)) <= 256, name
    for name in HEADLINE:
        assert name not in TOLERATED and int(kernels[name].get(".private_segment_fixed_size", 0)) == 0
