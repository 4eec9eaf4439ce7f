#!/usr/bin/env python3
"""tools/bandpass_probe.py : one BandpassEngine.accumulate_raw of the headline block -- 2^29 CASPSR samples (two polarisations,
1 GiB of bytes) at resolution 1024 -- timed with events after a warm-up; reports GB/s of input read, next to the library's build id.

  bandpass_probe.py [--log2-samples 29] [--resolution 1024] [--repeat 5] [--npol-out 2]

DESIGN.md 5 states the copy rate of this chip to compare with."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=29)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--npol-out", type=int, default=2)
    a = ap.parse_args(argv)
    import torch
    import dspsr_amd
    from dspsr_amd import _lib
    ndat = 1 << a.log2_samples
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    raw = torch.randint(-100, 100, (2 * ndat,), dtype=torch.int8, device="cuda")
    eng = dspsr_amd.BandpassEngine(ctx)
    eng.set_shape(1, 2, 1, a.resolution, a.npol_out)
    scale = dspsr_amd.eight_bit_scale()
    eng.accumulate_raw(raw, ndat, _lib.RAW_CASPSR, scale)            # warm-up (module load, LDS attribute, partial arrays)
    ctx.synchronize()
    times = []
    for _ in range(a.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.accumulate_raw(raw, ndat, _lib.RAW_CASPSR, scale)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    band = eng.synch()
    assert band[:2].min() > 0                                    # every channel of both polarisations received power
    times.sort()
    med = times[len(times) // 2]
    tp, tps, nseg = dspsr_amd.bandpass_check_input(1, 2, 1, a.resolution, _lib.RAW_CASPSR, 0, 0, 0, ndat)
    print(json.dumps({"probe": "bandpass accumulate_raw CASPSR", "build_id": dspsr_amd.build_id(), "samples": ndat, "bytes": 2 * ndat,
                      "resolution": a.resolution, "npol_out": a.npol_out, "parts_per_tile": tp, "tiles_per_segment": tps,
                      "segments": nseg, "ms_median": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4),
                      "GB_per_s_input": round(2 * ndat / med / 1e6, 1)}))
    eng.close()
    ctx.close()


if __name__ == "__main__":
    main()
