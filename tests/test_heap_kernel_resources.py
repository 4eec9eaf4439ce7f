"""The heap loader of the one-pass convolution (csrc/fb_conv1.hip, k_conv1_heaps<LOGM>) holds the raw 16-bit words of a tile where
the float kernel k_conv1<LOGM> holds float pairs: for every n_fft = 2^6 ... 2^13 it must exist in the SHIPPED library, use no more
scratch memory than the float instantiation of the same LOGM in the same library (k_conv1<13> is tolerated at 20 bytes,
tests/test_kernel_resources.py) and at most 256 VGPRs; the unpacker k_unpack_heaps uses no scratch.  Read from the code-object
metadata as tests/test_kernel_resources.py does.  CPU only: nothing is launched."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture)


@pytest.mark.parametrize("logm", range(6, 14))
def test_heap_loader_spills_no_more_than_the_float_kernel(kernels, logm):  # noqa: F811
    heap, flt = "k_conv1_heaps<%d>" % logm, "k_conv1<%d>" % logm
    assert heap in kernels, "%s is not in the library" % heap
    assert flt in kernels, "%s is not in the library" % flt
    h, f = kernels[heap], kernels[flt]
    hs, fs = int(h.get(".private_segment_fixed_size", 0)), int(f.get(".private_segment_fixed_size", 0))
    print(heap, "vgprs", h.get(".vgpr_count"), "scratch", hs, "|", flt, "vgprs", f.get(".vgpr_count"), "scratch", fs)
    assert hs <= fs, "%s uses %d bytes of scratch per lane, %s %d" % (heap, hs, flt, fs)
    assert int(h.get(".vgpr_count", 0)) <= 256


def test_unpacker_uses_no_scratch(kernels):  # noqa: F811
    assert "k_unpack_heaps" in kernels
    kd = kernels["k_unpack_heaps"]
    assert int(kd.get(".private_segment_fixed_size", 0)) == 0
    assert int(kd.get(".vgpr_count", 0)) <= 256
