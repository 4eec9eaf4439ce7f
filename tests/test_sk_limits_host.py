"""dspsr_amd.sk_limits (csrc/host_prep.cpp: the port of SKLimits::calc_limits, PearsonIV, Romberg / Neville, NewtonRaphson) against
tests/golden/sk_limits.json, the table the reference's own dsp::SKLimits gave for M in {32 ... 65536} x std_devs 1 ... 6 (double as
hex() and rounded to float32; failed_cf / failed_ccf where the reference reported a failed Newton iteration).  No device."""
import numpy as np
import pytest

import dspsr_amd
from sk_cases import golden_limits

TABLE = golden_limits()
KEYS = sorted(TABLE)


def _ulps(a, b):
    """distance of two positive float32 in units of the last place"""
    return abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32)))


def test_the_table_is_the_one_the_issue_describes():
    assert len(KEYS) == 16 * 6 and {m for m, _ in KEYS} == {32, 64, 100, 128, 256, 384, 512, 640, 1024, 2048, 4096, 8192, 16384, 32767,
                                                            32768, 65536}
    for key, lo, hi in (((128, 3), 0.601903975, 1.76296842), ((1024, 3), 0.834186196, 1.21695483), ((65536, 3), 0.9765625, 1.0234375)):
        assert (np.float32(TABLE[key]["lower_f32"]), np.float32(TABLE[key]["upper_f32"])) == (np.float32(lo), np.float32(hi))
    for r in TABLE.values():                                   # the float32 column is the double rounded
        assert np.float32(float.fromhex(r["lower_hex"])).view(np.uint32) == r["lower_f32_bits"]
        assert np.float32(float.fromhex(r["upper_hex"])).view(np.uint32) == r["upper_f32_bits"]
    assert TABLE[(1024, 6)]["failed_cf"] and np.float32(TABLE[(1024, 6)]["lower_f32"]) == np.float32(0.625)


@pytest.mark.parametrize("M,std_devs", KEYS)
def test_limits_within_one_ulp_of_the_reference(M, std_devs):
    """Newton's precision of 1e-12 lies far below float32's 6e-8: only a root on a rounding boundary can differ, and then by one."""
    r = TABLE[(M, std_devs)]
    lo, hi = dspsr_amd.sk_limits(M, std_devs)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert _ulps(lo, np.uint32(r["lower_f32_bits"]).view(np.float32)) <= 1, (lo, r["lower_f32"])
    assert _ulps(hi, np.uint32(r["upper_f32_bits"]).view(np.float32)) <= 1, (hi, r["upper_f32"])


def test_a_failed_iteration_falls_back_to_the_starting_guess():
    failed = [k for k in KEYS if TABLE[k]["failed_cf"] or TABLE[k]["failed_ccf"]]
    assert failed and (1024, 6) in failed
    for M, s in failed:
        r = TABLE[(M, s)]
        lo, hi = dspsr_amd.sk_limits(M, s)
        factor = np.sqrt(4.0 / M) * s
        if r["failed_cf"]:
            assert lo == np.float32(1 - factor) and lo.view(np.uint32) == r["lower_f32_bits"]
        if r["failed_ccf"]:
            assert hi == np.float32(1 + factor) and hi.view(np.uint32) == r["upper_f32_bits"]


def test_the_gaussian_branch_from_32768():
    for M in (32768, 65536):
        for s in range(1, 7):
            lo, hi = dspsr_amd.sk_limits(M, s)
            factor = np.sqrt(4.0 / M) * s
            assert (lo, hi) == (np.float32(1.0 - factor), np.float32(1.0 + factor))


@pytest.mark.parametrize("M,std_devs", [(0, 3), (2, 3), (24, 3), (31, 3), (128, 0)])
def test_refusals(M, std_devs):
    with pytest.raises(dspsr_amd.DspsrAmdError, match="M=%d < 32 or std_devs=%d == 0" % (M, std_devs)):
        dspsr_amd.sk_limits(M, std_devs)
