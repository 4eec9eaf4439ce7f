"""The instantiations of the Coherence search epilogue -- k_inv_chan<LOGF, 18 | 22, LOGT> (fb_inv_chan_search_coh.hip) and
k_rows_inv<LOGM, LOGFB, 4> (fb_two_pass.hip) -- in the SHIPPED library, from the AMDGPU metadata test_kernel_resources reads: every
one is there, fits the register file, and spills no more than its square-law sibling of the same LOGF / LOGT (k_inv_chan<LOGF,
2 | 6, LOGT>, k_rows_inv<., ., 2>), whose body it is but for four staged floats per sample in place of one or two.  The one the
digifits shape -F 4096:D on 400 MHz runs, k_inv_chan<12, ., 2>, uses no scratch at all.  CPU only: nothing is launched."""
import re

import pytest

from test_kernel_resources import kernels                                            # noqa: F401  (the module-scoped fixture)

MAX_LOGF = 13


def _full_logt(logf):
    """csrc/fb_common.h full_logt"""
    return 14 - logf if 14 - logf >= 1 else -1


# (new name, sibling): EPIP 18 = search + Coherence, 22 = the same on the pre-split spectrum; siblings 2 and 6
INV_CHAN = [("k_inv_chan<%d, %d, %d>" % (logf, epip, logt), "k_inv_chan<%d, %d, %d>" % (logf, epip - 16, logt))
            for logf in range(MAX_LOGF + 1) for epip in (18, 22) for logt in sorted({-1, _full_logt(logf)})]
ROWS_INV = [("k_rows_inv<%d, %d, 4>" % (m, 13 - m), "k_rows_inv<%d, %d, 2>" % (m, 13 - m)) for m in (9, 10, 11, 12)]


def _scratch(kd):
    return int(kd.get(".private_segment_fixed_size", 0))


@pytest.mark.parametrize("name,sibling", INV_CHAN + ROWS_INV, ids=[n for n, _ in INV_CHAN + ROWS_INV])
def test_the_coherence_form_is_shipped_and_no_heavier_than_its_sibling(kernels, name, sibling):       # noqa: F811
    assert name in kernels, "%s is not in the library" % name
    assert sibling in kernels, "%s is not in the library (renamed? this test names it)" % sibling
    kd, sd = kernels[name], kernels[sibling]
    assert int(kd.get(".vgpr_count", 0)) <= 256
    assert _scratch(kd) <= _scratch(sd), "%s: %d bytes of scratch per lane, %s has %d" % (name, _scratch(kd), sibling, _scratch(sd))
    assert int(kd.get(".group_segment_fixed_size", 0)) == int(sd.get(".group_segment_fixed_size", 0))


def test_the_family_is_exactly_these(kernels):                                       # noqa: F811
    """no instantiation of the new forms beyond the tables of fb_pick3c and fb_pick_rinv, and none missing"""
    got = {n for n in kernels if re.fullmatch(r"k_inv_chan<\d+, (18|22), -?\d+>|k_rows_inv<\d+, \d+, 4>", n)}
    assert got == {n for n, _ in INV_CHAN + ROWS_INV}
    assert len(got) == 60


@pytest.mark.parametrize("epip", [18, 22])
def test_the_digifits_shape_uses_no_scratch(kernels, epip):                          # noqa: F811
    assert _scratch(kernels["k_inv_chan<12, %d, 2>" % epip]) == 0
