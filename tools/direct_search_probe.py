#!/usr/bin/env python3
"""tools/direct_search_probe.py : the one-pass search front end (dspsr_amd.detect_raw) against the unfused chain of the same
library (unpack_fpt -> detect_square_law -> tscrunch_fpt) on one 256 MiB dual-polarisation block, Intensity.

One process, one stream; every figure is the median of --steps launches timed with device events after --warmup untimed ones.
  algorithmic bandwidth = (bytes of the block + 4 * nchan * npol_out * nout bytes written) / time, for both forms (what the
  unfused chain moves on top of that -- 16 B per (channel, sample) written and read again, 4 B detected written and read -- is
  its cost, not its work)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(torch, fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mib", type=int, default=256, help="block size")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nchan", type=int, nargs="*", default=[8, 64, 1024, 4096])
    ap.add_argument("--tscrunch", type=int, nargs="*", default=[1, 16])
    a = ap.parse_args(argv)
    import torch

    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    nbytes = a.mib << 20
    raw = torch.randint(-128, 128, (nbytes,), dtype=torch.int8, device="cuda")
    scale = dspsr_amd.eight_bit_scale()
    eng = dspsr_amd.DetectionEngine(ctx)
    print("# device %s, library %s, block %d MiB, median (min .. max) of %d launches after %d" % (
        torch.cuda.get_device_name(0), dspsr_amd.build_id(), a.mib, a.steps, a.warmup))
    print("# nchan tscrunch | detect_raw ms, GB/s | unpack + square_law + tscrunch ms (each), GB/s | ratio unfused / fused")
    for nchan in a.nchan:
        ndat = nbytes // (nchan * 4)
        volt = torch.empty((nchan, 2, 2 * ndat), dtype=torch.float32, device="cuda")
        det = torch.empty((nchan, 1, ndat), dtype=torch.float32, device="cuda")
        for ts in a.tscrunch:
            nout = ndat // ts
            out = torch.empty((nchan, 1, nout), dtype=torch.float32, device="cuda")
            carry = torch.zeros((nchan, 1), dtype=torch.float32, device="cuda")
            work = nbytes + 4 * nchan * nout
            f = timed(torch, lambda: dspsr_amd.detect_raw(ctx, raw, out, carry, 0, nchan, 2, ts, dspsr_amd.INTENSITY, scale), a.warmup, a.steps)
            fused = out.clone()
            u1 = timed(torch, lambda: dspsr_amd.unpack_fpt(ctx, raw, volt, nchan, 2, 2, scale), a.warmup, a.steps)
            u2 = timed(torch, lambda: eng.square_law(volt, det, intensity=True), a.warmup, a.steps)
            u3 = timed(torch, lambda: dspsr_amd.tscrunch_fpt(ctx, det, out, ts, carry, 0), a.warmup, a.steps)

            def chain():
                dspsr_amd.unpack_fpt(ctx, raw, volt, nchan, 2, 2, scale)
                eng.square_law(volt, det, intensity=True)
                dspsr_amd.tscrunch_fpt(ctx, det, out, ts, carry, 0)
            u = timed(torch, chain, a.warmup, a.steps)
            same = bool(torch.equal(fused, out))
            print("%5d %4d | %8.3f (%.3f .. %.3f) %7.1f | %8.3f (%.3f .. %.3f) = %.3f + %.3f + %.3f  %7.1f | %5.2f  %s" % (
                nchan, ts, f[0], f[1], f[2], work / f[0] / 1e6, u[0], u[1], u[2], u1[0], u2[0], u3[0], work / u[0] / 1e6, u[0] / f[0],
                "bit-identical" if same else "DIFFERENT"))
            del out
        del volt, det
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
