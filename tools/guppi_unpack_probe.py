#!/usr/bin/env python3
"""tools/guppi_unpack_probe.py : rate of dspsr_amd_unpack_guppi_fpt (k_unpack_guppi) beside k_unpack_heaps on the same number of
bytes -- both read 1 byte and write 4 per value -- at runs that are 16-byte aligned and at runs that are not
(block_nsamp odd, OVERLAP 2: the runs start on 4-byte boundaries only).

Alternating windows of the three calls, device events around each window, the first window of each discarded; the best and the
median window reported.  With --file-mib N a raw file of N MiB is written to --dir and folded: the wall time of dada.fold_file, and
on its engine the time of perform_detect per block from the RAW_GUPPI block against the same samples handed over as float rows
(the engine's own time: what a loader inside the forward pass could save at most).

  guppi_unpack_probe.py [--nchan 64] [--log2-ndat 20] [--nblock 4] [--windows 9] [--calls 10] [--file-mib 64] [--dir .] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def card(key, v):
    text = ("%-8s= '%-8s'" % (key, v)) if isinstance(v, str) else "%-8s= %20s" % (key, repr(v) if isinstance(v, float) else "%d" % v)
    return text.encode("ascii").ljust(80)


def write_raw(path, nchan, block_nsamp, nblock, seed=3):
    """a raw file of noise: nblock blocks of nchan runs of block_nsamp dual-polarisation samples, no overlap"""
    import numpy as np
    rng = np.random.default_rng(seed)
    blocsize = nchan * block_nsamp * 4
    cards = {"BACKEND": "GUPPI", "TELESCOP": "GBT", "FRONTEND": "Rcvr_800", "SRC_NAME": "noise", "RA_STR": "00:00:00.0", "DEC_STR": "+00:00:00.0",
             "FD_POLN": "LIN", "OBSFREQ": 820.0, "OBSBW": -100.0, "OBSNCHAN": nchan, "NPOL": 4, "NBITS": 8, "TBIN": nchan / 100e6, "PKTFMT": "1SFA",
             "PKTSIZE": blocsize // 16, "OVERLAP": 0, "BLOCSIZE": blocsize, "STT_IMJD": 55555, "STT_SMJD": 0, "STT_OFFS": 0.0}
    with open(path, "wb") as f:
        for k in range(nblock):
            f.write(b"".join(card(key, v) for key, v in dict(cards, PKTIDX=16 * k).items()) + b"END".ljust(80))
            f.write(rng.integers(-40, 40, blocsize, dtype=np.int8).tobytes())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nchan", type=int, default=64)
    ap.add_argument("--log2-ndat", type=int, default=20, help="samples per channel and polarisation of one call")
    ap.add_argument("--nblock", type=int, default=4, help="raw blocks the samples of a call lie in")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10, help="calls per window")
    ap.add_argument("--file-mib", type=int, default=64, help="0: no file")
    ap.add_argument("--dir", default=".")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import dspsr_amd
    if not torch.cuda.is_available():
        sys.exit("guppi_unpack_probe: no HIP device")
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    nchan, npol, ndat = a.nchan, 2, 1 << a.log2_ndat
    rng = np.random.default_rng(1)
    noise = torch.from_numpy(rng.integers(-128, 128, 1 << 24, dtype=np.int8)).cuda()
    rows = torch.empty((nchan, npol, 2 * ndat), dtype=torch.float32, device="cuda")

    def fill(nbytes):
        return noise.repeat(-(-nbytes // noise.numel()))[:nbytes].contiguous()
    # aligned: runs of block_nsamp = ndat / nblock samples, no overlap; unaligned: one sample fewer kept and OVERLAP 2 behind them
    geoms = {}
    for name, (bn, ovl) in (("guppi_aligned", (ndat // a.nblock, 0)), ("guppi_unaligned", (ndat // a.nblock - 1, 2))):
        cs = (bn + ovl) * 2 * npol
        lay = dspsr_amd.GuppiLayout(nchan, npol, bn, 0, cs, nchan * cs)
        n = a.nblock * bn
        geoms[name] = (fill(a.nblock * nchan * cs), lay, n)
        assert (cs % 16 == 0) == (name == "guppi_aligned")
    heaps = fill(ndat * nchan * npol * 2)
    calls = {name: (lambda g=g: dspsr_amd.unpack_guppi_fpt(ctx, g[0], rows, g[1], g[2])) for name, g in geoms.items()}
    calls["heaps"] = lambda: dspsr_amd.unpack_heaps_fpt(ctx, heaps, rows, nchan, npol, dspsr_amd.RAW_MEERKAT, 1.0, ndat=ndat)
    values = {name: g[2] * nchan * npol * 2 for name, g in geoms.items()}
    values["heaps"] = ndat * nchan * npol * 2

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / a.calls
    t = {name: [] for name in calls}
    for w in range(a.windows + 1):
        for name, fn in calls.items():
            dt = window(fn)
            if w:                                                    # the first window of each is the warm-up
                t[name].append(dt)
    res = {"nchan": nchan, "npol": npol, "ndat": ndat, "nblock": a.nblock, "build_id": dspsr_amd.build_id()}
    for name in calls:
        best, med, worst = min(t[name]), sorted(t[name])[len(t[name]) // 2], max(t[name])
        res[name] = {"values": values[name], "best_s": best, "median_s": med, "worst_s": worst,
                     "GB_per_s_read_plus_written": 5 * values[name] / med / 1e9, "best_GB_per_s": 5 * values[name] / best / 1e9}
    for name in geoms:
        res[name]["rate_over_heaps_median"] = res[name]["GB_per_s_read_plus_written"] / res["heaps"]["GB_per_s_read_plus_written"]
    ctx.close()
    if a.file_mib:
        res["file"] = fold_file_times(a, dspsr_amd, torch, np)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def fold_file_times(a, dspsr_amd, torch, np):
    from dspsr_amd import dada, guppi, pipeline
    nchan, M = a.nchan, 1024
    nblock = 4
    bn = (a.file_mib << 20) // (nblock * nchan * 4)
    path = os.path.join(a.dir, "guppi_unpack_probe.raw")
    write_raw(path, nchan, bn, nblock)
    cfg = pipeline.Config(nchan=nchan, dispersion_measure=5.0, nbin=256, folding_period=0.0123, freq_res=M, parts_per_block=128, max_parts=128)
    out = {"bytes": os.path.getsize(path), "nchan": nchan, "freq_res": M}
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        lt = dada.fold_file(path, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)
        walls.append(time.perf_counter() - t0)
        lt.close()
    out["fold_file_wall_s"] = walls                                  # (the first includes the first launches)
    # the engine alone, block by block: from the RAW_GUPPI block, and from the same samples as float rows
    f = guppi.GuppiFile(path)
    lt = pipeline.LoadToFold(cfg, f.info, device=0, stream=torch.cuda.current_stream().cuda_stream)
    blocks = [(torch.from_numpy(v).cuda(), n, first) for v, n, first in f.blocks(lt)]
    det = torch.empty((nchan, 1, 4 * cfg.parts_per_block * lt.nkeep), dtype=torch.float32, device="cuda")
    step = lt.nsamp_step
    t = {"raw": [], "rows": []}
    for w in range(4):
        for how in t:
            total = 0.0
            for raw, n, first in blocks:
                if how == "rows":
                    x, in_step = lt.fb.unpack_guppi(raw, first, n)
                    lt.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if how == "raw":
                    lt.fb.perform_detect(det, n, dspsr_amd.COHERENCE, 4, raw=raw, layout=dspsr_amd.guppi_at(first))
                else:
                    lt.fb.perform_detect(det, n, dspsr_amd.COHERENCE, 4, inp=x, in_step=2 * step)
                e1.record()
                e1.synchronize()
                total += e0.elapsed_time(e1) * 1e-3
            if w:
                t[how].append(total)
    lt.close()
    os.remove(path)
    out["perform_detect_s"] = {how: {"best": min(v), "median": sorted(v)[len(v) // 2]} for how, v in t.items()}
    out["unpack_share_of_raw"] = 1.0 - out["perform_detect_s"]["rows"]["median"] / out["perform_detect_s"]["raw"]["median"]
    return out


if __name__ == "__main__":
    main()
