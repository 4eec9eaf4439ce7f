"""k_bandpass and k_plfb over seeded noise (tests/spectral_sums_cases.py) against tests/golden/spectral_sums_parent.json: the digest
of the sums, for equality.  The fixture was recorded with tools/spectral_sums_record.py on the MI355X from the commit in front of the
one that moved the two kernels' shared transform-detect tile into csrc/spectral_tile.h (two recordings, equal).  The tone tests hold
sums that are exact in any order and the noise tests allow four times the float32 error: only this one notices a reordered sum."""
import json
import os

import pytest

import dspsr_amd
import spectral_sums_cases as cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_sums_parent.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.mark.parametrize("name", cases.IDS)
def test_sums_keep_the_parents_bits(ctx, name):
    got = cases.record_of(cases.run_case(dspsr_amd, ctx, name))
    want = GOLDEN[name]
    print("%s first values %s, recorded %s" % (name, got["first"], want["first"]))
    assert got["shape"] == want["shape"]
    assert got["sha256"] == want["sha256"]
