"""The condition the `dspsr -R` pipeline tests rest on (tests/test_gpu_rfi_pipeline.py), checked on the same bytes without a device:
the float32 and the float64 restatement give the same mask, and in no round does any channel's statistic lie within 1e-3 relative
of its cutoff, or a neighbour difference within 1e-3 of twice the cutoff -- so a passband that differs from the restatement's by
float32 rounding gives the same mask.  CPU only."""
import numpy as np

import rfi_pipeline_case as pc
import rfi_reference as rr


def test_the_stream_decides_its_mask_with_room(oracle):
    plan = pc.plan(oracle)
    assert (plan.freq_res, plan.nchan_subband) == (pc.FREQ_RES, pc.NCHAN) and pc.blocks_used() == 8
    raw = pc.stream(plan.nsamp_step, plan.nsamp_overlap)
    assert raw.size == 2 * (pc.NBLOCK * pc.PARTS * plan.nsamp_step + plan.nsamp_overlap)
    band32, r32 = pc.restatement(raw, np.float32)
    band64, r64 = pc.restatement(raw, np.float64)
    print("rounds %d, zapped %d, margin f32 %.3e f64 %.3e" % (r32["rounds"], r32["total_zapped"], r32["margin"], r64["margin"]))
    assert np.array_equal(r32["mask"], r64["mask"]) and r32["rounds"] == r64["rounds"] and not r32["endless"]
    assert r32["margin"] >= 1e-3 and r64["margin"] >= 1e-3
    assert np.abs(band32 - band64).max() <= 1e-5 * band64.max()
    zapped = set(np.flatnonzero(r32["mask"] == 0))
    assert {k for k, *_ in pc.TONES} <= zapped and len(zapped) < 32
    # the literal loop zaps the same channels in p0 / p1 and leaves a mask of ones
    _, lit = pc.restatement(raw, np.float32, keep_zapped=False)
    assert np.all(lit["mask"] == 1) and set(np.flatnonzero(lit["p0"] == 0)) == zapped
    # the product: required = 16 x 256 = 4 x 1024
    ph = rr.rfi_expand(r32["mask"], pc.NCHAN * pc.FREQ_RES)
    assert np.array_equal(ph.real.reshape(1024, 4)[:, 0], r32["mask"]) and ph.size == 4096
