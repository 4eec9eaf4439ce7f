"""The kernels of csrc/fold_moments.hip -- dsp::FourthMoment and the moments fold with both loaders, exact and LONG -- use no
scratch memory, and their LDS (static: the code object states it) stays within the 64 KiB a fold kernel may ask for without
raising the dynamic-LDS attribute, which no fold kernel does.  Read from the AMDGPU metadata of the shipped library, as
tests/test_kernel_resources.py does.  CPU only."""
import subprocess

import pytest

import moments_cases as mc
from test_kernel_resources import LIB, _code_objects, _kernels

# kernel -> bytes of LDS it declares: the chunk image, and for LONG the 14 sums of each of its micro-blocks
MOMENTS = {
    "k_fourth_moment": mc.MOM_FM_SAMPLES * mc.MOM_NDIM * 4,
    "k_fold_moments<true, false>": mc.MOM_CHUNK_STOKES * 4 * 4,                  # (the unused one-float array of the exact variants is dropped)
    "k_fold_moments<true, true>": mc.MOM_CHUNK_STOKES * 4 * 4 + mc.MOM_CHUNK_STOKES // mc.MOM_MB * mc.MOM_NDIM * 4,
    "k_fold_moments<false, false>": mc.MOM_CHUNK_STREAM * mc.MOM_NDIM * 4,
    "k_fold_moments<false, true>": mc.MOM_CHUNK_STREAM * mc.MOM_NDIM * 4 + mc.MOM_CHUNK_STREAM // mc.MOM_MB * mc.MOM_NDIM * 4,
}
FOLD_LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for co in _code_objects(open(LIB, "rb").read()):
        ks.update(_kernels(co))
    names = sorted(ks)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d.split("(")[0].replace("void dspsr_amd::", "").replace("dspsr_amd::", ""): ks[n] for d, n in zip(dem, names)}


@pytest.mark.parametrize("name", sorted(MOMENTS))
def test_moments_kernels_use_no_scratch(kernels, name):
    assert name in kernels, "kernel %s not in the library" % name
    kd = kernels[name]
    assert int(kd.get(".private_segment_fixed_size", 0)) == 0, "%s spills %s bytes per lane" % (name, kd.get(".private_segment_fixed_size"))
    # 128 VGPRs: four 256-thread workgroups per compute unit (the occupancy the bins-per-thread choice is made for)
    assert int(kd.get(".vgpr_count", 0)) + int(kd.get(".agpr_count", 0)) <= 128
    lds = int(kd.get(".group_segment_fixed_size", 0))
    assert lds == MOMENTS[name] <= FOLD_LDS_LIMIT
    assert 4 * lds <= 160 * 1024                       # and four of them fit the 160 KiB of a compute unit
