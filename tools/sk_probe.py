#!/usr/bin/env python3
"""tools/sk_probe.py : the three steps of SpectralKurtosisEngine on rows of Gaussian noise -- compute, the detection chain and the
in-place mask -- each timed with events after a warm-up, next to dspsr_amd_copy_fpt of the same rows (a plain read and write of
them) and the library's build id.

  sk_probe.py [--nchan 1024] [--npol 2] [--log2-ndat 16] [-M 128] [--repeat 7] [--zap 0.05]

--zap: the fraction of channels made constant in modulus (tscr and skfb zap them) so that the mask has something to zero.  GB/s count the bytes of
the rows once for compute, twice for the copy; the mask writes only what it zaps."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, repeat):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=1024)
    ap.add_argument("--npol", type=int, default=2)
    ap.add_argument("--log2-ndat", type=int, default=16)
    ap.add_argument("-M", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--zap", type=float, default=0.05)
    a = ap.parse_args(argv)
    import torch
    import dspsr_amd
    ndat = 1 << a.log2_ndat
    npart = ndat // a.M
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.randn((a.nchan, a.npol, 2 * ndat), generator=gen, device="cuda", dtype=torch.float32)
    view = rows[:, :, :2 * npart * a.M].view(a.nchan, a.npol, npart, 2 * a.M)
    view[torch.rand(a.nchan, generator=gen, device="cuda") < a.zap] = 1.0
    keep = rows.clone()
    other = torch.empty_like(rows)
    eng = dspsr_amd.SpectralKurtosisEngine(ctx)
    eng.set_shape(a.nchan, a.npol, a.M)
    eng.set_options(3)
    lim, lim_t = dspsr_amd.sk_limits(a.M, 3), dspsr_amd.sk_limits(a.M * npart, 3)

    def detect():
        eng.reset_mask()
        eng.detect_tscr(*lim_t)
        eng.detect_skfb(*lim)
        eng.detect_fscr()
        eng.count_zapped()

    def mask():                                               # (zeros over zeros after the first call: the same stores)
        eng.mask(rows, rows)
    nbytes = rows.numel() * 4
    t_copy = timed(lambda: dspsr_amd.copy_data_fpt(ctx, other, rows), a.repeat)
    t_compute = timed(lambda: eng.compute(rows, ndat), a.repeat)
    t_detect = timed(detect, a.repeat)
    zapped = float(eng.zapmask().mean())
    t_mask = timed(mask, a.repeat)
    rows.copy_(keep)
    t_all = timed(lambda: eng.transform(rows, rows, ndat), a.repeat)
    print(json.dumps({"probe": "spectral kurtosis", "build_id": dspsr_amd.build_id(), "nchan": a.nchan, "npol": a.npol, "ndat": ndat, "M": a.M,
                      "row_bytes": nbytes, "zapped_fraction": round(zapped, 4),
                      "copy_fpt_ms": [round(t, 4) for t in t_copy], "copy_fpt_GB_per_s": round(2 * nbytes / t_copy[0] / 1e6, 1),
                      "compute_ms": [round(t, 4) for t in t_compute], "compute_GB_per_s": round(nbytes / t_compute[0] / 1e6, 1),
                      "detect_ms": [round(t, 4) for t in t_detect], "mask_in_place_ms": [round(t, 4) for t in t_mask],
                      "mask_GB_per_s_written": round(zapped * nbytes / t_mask[0] / 1e6, 1),
                      "transform_ms": [round(t, 4) for t in t_all], "ms_order": "median, min, max"}))
    eng.close()
    ctx.close()


if __name__ == "__main__":
    main()
