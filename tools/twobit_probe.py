#!/usr/bin/env python3
"""tools/twobit_probe.py : time of dspsr_amd_twobit_unpack (k_twobit_levels + k_twobit_unpack) per input byte, beside k_unpack_heaps
at the same output bytes -- both write 4 bytes per real sample and should sit at the same store rate.

Alternating windows of the two calls, device events around each window, the best and the median window reported.  Under
`rocprofv3 --kernel-trace --stats -- python tools/twobit_probe.py --windows 3` the kernel table splits the two-bit call into its
two kernels.

  twobit_probe.py [--log2-ndat 25] [--nsample 512] [--npol 2] [--windows 9] [--calls 20] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-ndat", type=int, default=25, help="samples per digitiser of one call")
    ap.add_argument("--nsample", type=int, default=512)
    ap.add_argument("--npol", type=int, default=2)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20, help="calls per window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import dspsr_amd
    from dspsr_amd import twobit
    if not torch.cuda.is_available():
        sys.exit("twobit_probe: no HIP device")
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    ndat, npol, nsample = 1 << a.log2_ndat, a.npol, a.nsample
    nlow_min, nlow_max = twobit.limits(nsample)
    levels = torch.from_numpy(twobit.levels(nsample, nlow_min, nlow_max)).cuda()
    # noise at the optimal threshold: two thirds of the samples low, every window kept
    rng = np.random.default_rng(1)
    x = rng.standard_normal(1 << 22)
    code = np.where(x < 0, np.where(np.abs(x) >= twobit.THRESHOLD, 0, 1), np.where(np.abs(x) >= twobit.THRESHOLD, 3, 2)).astype(np.uint8).reshape(-1, 4)
    tile = (code[:, 0] << 6) | (code[:, 1] << 4) | (code[:, 2] << 2) | code[:, 3]
    nbyte = ndat // 4 * npol
    raw = torch.from_numpy(np.resize(tile, nbyte)).cuda()
    rows = torch.empty((npol, ndat), dtype=torch.float32, device="cuda")
    weights = torch.empty((npol, ndat // nsample), dtype=torch.int32, device="cuda")
    # the yardstick: heaps of one channel, the same number of output floats
    hdat = ndat // 2                                             # complex samples per polarisation
    heaps = torch.from_numpy(rng.integers(-128, 128, hdat * 2 * npol, dtype=np.int8)).cuda()
    hrows = torch.empty((1, npol, 2 * hdat), dtype=torch.float32, device="cuda")

    def two():
        dspsr_amd.twobit_unpack(ctx, raw, rows, levels, weights, nsample, nlow_min, nlow_max, dspsr_amd.TWOBIT_OFFSET_BINARY, 0, ndat)

    def heap():
        dspsr_amd.unpack_heaps_fpt(ctx, heaps, hrows, 1, npol, dspsr_amd.RAW_MEERKAT, 1.0, ndat=hdat)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / a.calls
    for fn in (two, heap):
        window(fn)                                               # warm-up
    assert int(weights.sum()) == weights.numel(), "the probe's noise must keep every window"
    t = {"twobit": [], "heaps": []}
    for _ in range(a.windows):
        t["twobit"].append(window(two))
        t["heaps"].append(window(heap))
    out_bytes = 4 * ndat * npol
    res = {"ndat": ndat, "npol": npol, "nsample": nsample, "output_bytes": out_bytes, "build_id": dspsr_amd.build_id()}
    for name, in_bytes in (("twobit", nbyte), ("heaps", heaps.numel())):
        best, med = min(t[name]), sorted(t[name])[len(t[name]) // 2]
        res[name] = {"input_bytes": in_bytes, "best_s": best, "median_s": med, "ps_per_input_byte": 1e12 * best / in_bytes,
                     "output_GB_per_s": out_bytes / best / 1e9, "median_output_GB_per_s": out_bytes / med / 1e9}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
