"""The SIGPROC unpacker k_unpack_sigproc<NBIT, LW> (csrc/unpack_sigproc.hip) is a transpose through LDS: every body -- one per
sample size NBIT and load width LW -- must exist in the SHIPPED library, use no scratch memory and at most 256 VGPRs.  Read from the
code-object metadata as tests/test_kernel_resources.py does.  CPU only: nothing is launched."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture)

# load widths per sample size: 16, 8, 4, 2 or 1 bytes, at least one value, at most an eighth of the tile's 16 * NBIT bytes
BODIES = {1: (1, 2), 2: (1, 2, 4), 4: (1, 2, 4, 8), 8: (1, 2, 4, 8, 16), 16: (2, 4, 8, 16), 32: (4, 8, 16)}


@pytest.mark.parametrize("nbit", sorted(BODIES))
def test_sigproc_unpacker_is_shipped_and_uses_no_scratch(kernels, nbit):  # noqa: F811
    for lw in BODIES[nbit]:
        name = "k_unpack_sigproc<%d, %d>" % (nbit, lw)
        assert name in kernels, "%s is not in the library" % name
        kd = kernels[name]
        print(name, "vgprs", kd.get(".vgpr_count"), "sgprs", kd.get(".sgpr_count"), "scratch", kd.get(".private_segment_fixed_size", 0),
              "lds", kd.get(".group_segment_fixed_size", 0))
        assert int(kd.get(".private_segment_fixed_size", 0)) == 0
        assert int(kd.get(".vgpr_count", 0)) <= 256
        assert int(kd.get(".group_segment_fixed_size", 0)) == 128 * 64 * 4          # the tile image alone


def test_no_other_sigproc_unpacker_body(kernels):  # noqa: F811
    got = sorted(k for k in kernels if k.startswith("k_unpack_sigproc"))
    assert got == sorted("k_unpack_sigproc<%d, %d>" % (n, lw) for n in BODIES for lw in BODIES[n])
