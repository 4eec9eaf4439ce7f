"""The cyclic-fold kernels (csrc/cyclic_fold.hip) that the GPU tests and tools/cyclic_probe.py launch use no scratch memory and at
most 256 VGPRs: read from the AMDGPU metadata of the shipped library, as tests/test_kernel_resources.py does.  CPU only."""
import subprocess

import pytest

from test_kernel_resources import LIB, _code_objects, _kernels

CYCLIC = ["k_cyclic_fold<1, 1>", "k_cyclic_fold<2, 1>", "k_cyclic_fold<2, 2>", "k_cyclic_fold<2, 4>", "k_cyclic_combine"]


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for co in _code_objects(open(LIB, "rb").read()):
        ks.update(_kernels(co))
    names = sorted(ks)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d.split("(")[0].replace("void dspsr_amd::", "").replace("dspsr_amd::", ""): ks[n] for d, n in zip(dem, names)}


@pytest.mark.parametrize("name", CYCLIC)
def test_cyclic_kernels_use_no_scratch(kernels, name):
    assert name in kernels, "kernel %s not in the library" % name
    kd = kernels[name]
    assert int(kd.get(".private_segment_fixed_size", 0)) == 0, "%s spills %s bytes per lane" % (name, kd.get(".private_segment_fixed_size"))
    assert int(kd.get(".vgpr_count", 0)) <= 256
    assert int(kd.get(".group_segment_fixed_size", 0)) <= 64 * 1024
