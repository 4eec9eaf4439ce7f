"""The spectral-kurtosis kernels (csrc/sk.hip) use no scratch memory, and k_sk_compute few enough VGPRs for eight waves per SIMD (it
hides the latency of its few loads per lane with waves, not with registers): read from the AMDGPU metadata of the shipped library,
as tests/test_kernel_resources.py does.  CPU only."""
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


def test_every_kernel_is_there_and_spills_nothing(kernels):
    mine = {k: v for k, v in kernels.items() if k.startswith("k_sk_")}
    assert sorted(mine) == ["k_sk_compute<false>", "k_sk_compute<true>", "k_sk_count", "k_sk_detect_fscr", "k_sk_detect_skfb",
                            "k_sk_detect_tscr", "k_sk_mask", "k_sk_mask_zero", "k_sk_tscr"]
    for name, kd in mine.items():
        assert int(kd.get(".private_segment_fixed_size", 0)) == 0, "%s spills %s bytes per lane" % (name, kd.get(".private_segment_fixed_size"))
        assert int(kd.get(".group_segment_fixed_size", 0)) == 0, "%s uses LDS" % name
    for name in ("k_sk_compute<false>", "k_sk_compute<true>"):
        assert int(mine[name][".vgpr_count"]) <= 64, "%s: %s VGPRs" % (name, mine[name][".vgpr_count"])
