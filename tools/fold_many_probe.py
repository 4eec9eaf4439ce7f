#!/usr/bin/env python3
"""tools/fold_many_probe.py : dspsr_amd_fold_fold_many (P pulsars over ONE detected block, k_fold_many) against P x
dspsr_amd_fold_fold, timed with HIP events around the fold calls alone, at two detected shapes of the bench workloads:

  plain     dspsr -F 128 (k_fb_plain's detected rows): 128 channels x 1 pol x 2^20 samples x ndim 4 (a half block)
  headline  -F 1024:D -x 4096: 1024 channels x 1 pol x 64 x 3252 samples x ndim 4 (one 64-part block)

and two folding periods per shape: `dense` (a period of more than FOLD_CHUNK = 2048 samples: the per-chunk table) and `walk`
(a millisecond pulsar, fewer than 2048 samples per period: the interval walk).  Pulsar k folds with period * (1 + 0.013 k).
One JSON line per (shape, period, P): median ms of `reps` calls, Msamples/s per pulsar (samples of the block per call time),
and the detected bytes each form reads from HBM at least (fold_many: once per launch of at most 8 plans; the singles: P times).
Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = {"plain": (128, 1 << 20), "headline": (1024, 64 * 3252)}
# (samples per period, nbin): dense 34883 samples (the headline's Vela period at its detected rate) over 1024 bins;
# walk 640 samples (a 1.6 ms pulsar at 0.4 MHz) over 256 bins
PERIODS = {"dense": (34883.0, 1024), "walk": (640.0, 256)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="plain,headline")
    ap.add_argument("--pulsars", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    import dspsr_amd
    assert torch.cuda.is_available(), "fold_many_probe needs a HIP device"
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for shape in a.shapes.split(","):
        nchan, ndat = SHAPES[shape]
        rows = torch.rand((nchan, 1, ndat * 4), dtype=torch.float32, device="cuda")
        nbytes = rows.numel() * 4
        for kind, (spp, nbin) in PERIODS.items():
            for P in [int(p) for p in a.pulsars.split(",")]:
                engs = []
                for _ in range(P):
                    e = dspsr_amd.FoldEngine(ctx)
                    e.set_shape(nchan, 1, 4, nbin)
                    engs.append(e)

                def plan():
                    for k, e in enumerate(engs):
                        e.set_nbin(nbin)
                        e.set_ndat(ndat, 0)
                        e.set_bins(0.1 * k, 1.0 / (spp * (1 + 0.013 * k)), ndat, 0)
                res = {}
                for form in ("many", "single"):
                    ts = []
                    for r in range(a.reps + 1):                    # the first call warms up
                        plan()
                        torch.cuda.synchronize()
                        ev0.record()
                        if form == "many":
                            nshared = dspsr_amd.FoldEngine.fold_many(engs, rows)
                            assert nshared == (P if P > 1 else 0), (kind, nshared)   # (one plan: the single fold)
                        else:
                            for e in engs:
                                e.fold(rows)
                        ev1.record()
                        torch.cuda.synchronize()
                        if r:
                            ts.append(ev0.elapsed_time(ev1))
                    res[form] = statistics.median(ts)
                prof = [e.synch() for e in engs]
                for e in engs:
                    e.close()
                print(json.dumps(dict(shape=shape, period=kind, samples_per_period=spp, nbin=nbin, pulsars=P,
                                      ms_many=round(res["many"], 4), ms_singles=round(res["single"], 4),
                                      speedup=round(res["single"] / res["many"], 3),
                                      msamples_s_per_pulsar_many=round(nchan * ndat / (res["many"] * 1e3), 1),
                                      msamples_s_per_pulsar_singles=round(nchan * ndat / (res["single"] * 1e3), 1),
                                      gbytes_read_many=round((P + 7) // 8 * nbytes / 1e9, 3),
                                      gbytes_read_singles=round(P * nbytes / 1e9, 3),
                                      finite=bool(all(np.isfinite(p).all() for p in prof)))), flush=True)
        del rows
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
