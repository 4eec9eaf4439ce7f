#!/usr/bin/env python3
"""tools/fits_digitize_probe.py : one dspsr_amd.FITSDigitizer.pack of 4096 channels x 4 products x nsblk samples against the pair the
library already had for the same rows -- dspsr_amd.Rescale.digitize_fpt with the interval set to the block, i.e. its sums pass, its
update and its 64 x 64 LDS turn -- which moves the same bytes through the same tile.

One process, one stream.  The two forms alternate in windows of --window seconds (default 1 s): a window queues calls in batches of
--batch between two device events and ends with a synchronise; the figure of a window is its event time over its calls.  Every form
gets --rounds windows; the spread between the windows of the EXISTING pair is the margin a difference has to exceed.
  byte model per sample: 2 x 4 B read (the sums pass and the pack pass each read the float) + nbit / 8 B written."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def window(torch, fn, seconds, batch):
    """us per call over one window of at least `seconds`"""
    calls, ms, t0 = 0, 0.0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        ms += a.elapsed_time(b)
        calls += batch
    return 1e3 * ms / calls


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--npol", type=int, default=4)
    ap.add_argument("--nsblk", type=int, nargs="*", default=[2048, 8192])
    ap.add_argument("--nbit", type=int, nargs="*", default=[2, 8])
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM peak the achieved fraction is quoted against (MI355X: 8 TB/s)")
    ap.add_argument("--json", default=None, help="also write the record here")
    a = ap.parse_args(argv)
    import torch

    import dspsr_amd
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    record = dict(device=torch.cuda.get_device_name(0), build_id=dspsr_amd.build_id(), nchan=a.nchan, npol=a.npol, window_s=a.window,
                  rounds=a.rounds, cases=[])
    print("# device %s, library %s, %d channels x %d products; windows of %.1f s, %d per form, alternating" % (
        record["device"], record["build_id"], a.nchan, a.npol, a.window, a.rounds))
    print("# nsblk nbit | FITSDigitizer.pack us (min .. max of the windows) GB/s fraction | Rescale.digitize_fpt us (min .. max) GB/s | pack / pair")
    gen = torch.Generator(device="cuda").manual_seed(20151124)
    for nsblk in a.nsblk:
        rows = torch.randn((a.nchan, a.npol, nsblk), generator=gen, device="cuda", dtype=torch.float32) * 3.0 + 30.0
        ncol = a.nchan * a.npol
        scl, offs = (torch.empty(ncol, dtype=torch.float32, device="cuda") for _ in range(2))
        for nbit in a.nbit:
            out = torch.empty(nsblk * ncol * nbit // 8, dtype=torch.uint8, device="cuda")
            dig = dspsr_amd.FITSDigitizer(ctx, a.nchan, a.npol, nbit, nsblk)
            resc = dspsr_amd.Rescale(ctx, a.nchan, a.npol, nsblk)
            forms = {"pack": lambda: dig.pack(rows, out, scl, offs), "pair": lambda: resc.digitize_fpt(rows, out, nbit)}
            for fn in forms.values():                          # warm up both shapes
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            us = {k: [] for k in forms}
            for _ in range(a.rounds):
                for k, fn in forms.items():
                    us[k].append(window(torch, fn, a.window, a.batch))
            nbytes = nsblk * ncol * (8 + nbit / 8.0)
            med = {k: statistics.median(v) for k, v in us.items()}
            gbs = {k: nbytes / med[k] / 1e3 for k in med}
            case = dict(nsblk=nsblk, nbit=nbit, model_bytes=nbytes, pack_us=us["pack"], pair_us=us["pair"], pack_median_us=med["pack"],
                        pair_median_us=med["pair"], pack_gbs=gbs["pack"], pair_gbs=gbs["pair"], pack_fraction_of_peak=gbs["pack"] / a.peak_gbs,
                        pair_spread=(max(us["pair"]) - min(us["pair"])) / med["pair"], ratio=med["pack"] / med["pair"])
            record["cases"].append(case)
            print("%5d %2d | %8.1f (%8.1f .. %8.1f) %7.0f %.3f | %8.1f (%8.1f .. %8.1f) %7.0f | %.3f (spread of the pair %.3f)" % (
                nsblk, nbit, med["pack"], min(us["pack"]), max(us["pack"]), gbs["pack"], case["pack_fraction_of_peak"], med["pair"],
                min(us["pair"]), max(us["pair"]), gbs["pair"], case["ratio"], case["pair_spread"]))
            dig.close()
            resc.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(record, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
