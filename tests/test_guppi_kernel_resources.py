"""The GUPPI unpacker k_unpack_guppi (csrc/unpack_guppi.hip) is a streaming kernel: it must exist in the SHIPPED library, use no
scratch memory and at most 256 VGPRs.  Read from the code-object metadata as tests/test_kernel_resources.py does.  CPU only: nothing
is launched."""
from test_kernel_resources import kernels  # noqa: F401  (fixture)


def test_guppi_unpacker_is_shipped_and_uses_no_scratch(kernels):  # noqa: F811
    assert "k_unpack_guppi" in kernels, "k_unpack_guppi is not in the library"
    kd = kernels["k_unpack_guppi"]
    print("k_unpack_guppi vgprs", kd.get(".vgpr_count"), "sgprs", kd.get(".sgpr_count"), "scratch", kd.get(".private_segment_fixed_size", 0))
    assert int(kd.get(".private_segment_fixed_size", 0)) == 0
    assert int(kd.get(".vgpr_count", 0)) <= 256
