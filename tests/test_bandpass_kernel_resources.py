"""Every instantiation of the passband kernels (csrc/bandpass.hip) uses no scratch memory and at most 256 VGPRs (a workgroup of 512 threads is
two waves per SIMD): read from the AMDGPU metadata of the shipped library, as tests/test_kernel_resources.py does.  CPU only."""
import subprocess

import pytest

from test_kernel_resources import LIB, _code_objects, _kernels


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for co in _code_objects(open(LIB, "rb").read()):
        ks.update(_kernels(co))
    names = sorted(ks)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d.split("(")[0].replace("void dspsr_amd::", "").replace("dspsr_amd::", ""): ks[n] for d, n in zip(dem, names)}


def test_every_instantiation_is_there_and_spills_nothing(kernels):
    mine = {k: v for k, v in kernels.items() if k.startswith("k_bandpass")}
    # float rows and the generic 8-bit order: 13 lengths x 2 ndim x 3 npol_out each; CASPSR: 13 x (npol_out 2, 4); the combine
    assert len(mine) == 2 * 13 * 2 * 3 + 13 * 2 + 1, sorted(mine)
    assert "k_bandpass_combine" in mine
    for name, kd in mine.items():
        assert int(kd.get(".private_segment_fixed_size", 0)) == 0, "%s spills %s bytes per lane" % (name, kd.get(".private_segment_fixed_size"))
        assert int(kd.get(".vgpr_count", 0)) <= 256, "%s: %s VGPRs" % (name, kd.get(".vgpr_count"))
