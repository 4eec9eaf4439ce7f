"""The two kernels of csrc/twobit.hip exist in the SHIPPED library, k_twobit_unpack for one and two digitisers, and none of them
uses scratch memory: the sixteen values of a word stay in registers.  Read from the code-object metadata as
tests/test_kernel_resources.py does.  CPU only: nothing is launched."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture)


@pytest.mark.parametrize("name", ["k_twobit_levels", "k_twobit_unpack<1>", "k_twobit_unpack<2>"])
def test_twobit_kernels_use_no_scratch(kernels, name):  # noqa: F811
    assert name in kernels, "%s is not in the library" % name
    kd = kernels[name]
    print(name, "vgprs", kd.get(".vgpr_count"), "scratch", kd.get(".private_segment_fixed_size", 0))
    assert int(kd.get(".private_segment_fixed_size", 0)) == 0
    assert int(kd.get(".vgpr_count", 0)) <= 64
