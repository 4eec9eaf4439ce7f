#!/usr/bin/env python3
"""tools/sigproc_unpack_probe.py : rate of dspsr_amd_unpack_sigproc_fpt (k_unpack_sigproc) at every sample size, as achieved GB/s of
its byte model -- nbit / 8 bytes read and 4 written per value --, beside the yardstick k_unpack_guppi at the same
number of output bytes, which has the same 1 + 4 byte model at 8 bits but no transpose in it.

Shape: nchan 4096, npol 1, 2^16 spectra (2^28 values, 1 GiB of float rows); the yardstick: 64 channels x 2 polarisations x 2^20
complex samples.  The 8-bit case is also timed with the spectra starting one byte into the allocation (byte loads).

Alternating windows of all calls, device events around each window, the first window of each discarded; the best, the median and
the worst window reported: their spread is the run-to-run spread of the session.  With --file-mib N an 8-bit file of N MiB is
written to --dir and folded with -K: the wall time of dada.fold_file, and the time to read the file's bytes on the host beside it.

  sigproc_unpack_probe.py [--nchan 4096] [--log2-ndat 16] [--windows 9] [--calls 5] [--file-mib 64] [--dir .] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NBITS = (1, 2, 4, 8, 16, 32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--log2-ndat", type=int, default=16, help="spectra of one call")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5, help="calls per window")
    ap.add_argument("--file-mib", type=int, default=64, help="0: no file")
    ap.add_argument("--dir", default=".")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import dspsr_amd
    if not torch.cuda.is_available():
        sys.exit("sigproc_unpack_probe: no HIP device")
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    nchan, npol, ndat = a.nchan, 1, 1 << a.log2_ndat
    nvalue = nchan * npol * ndat
    rng = np.random.default_rng(1)
    # (finite floats when read as 32-bit values: exponent bytes below 0x7f)
    noise = torch.from_numpy(rng.integers(0, 0x70, 1 << 24, dtype=np.uint8)).cuda()
    rows = torch.empty((nchan, npol, ndat), dtype=torch.float32, device="cuda")

    def fill(nbytes, skew=0):
        return noise.repeat(-(-(nbytes + skew) // noise.numel()))[:nbytes + skew].contiguous()[skew:]
    calls, values, read_bytes = {}, {}, {}
    for nbit in NBITS:
        raw = fill(nvalue * nbit // 8)
        calls["nbit%d" % nbit] = lambda raw=raw, nbit=nbit: dspsr_amd.unpack_sigproc_fpt(ctx, raw, rows, nbit, nchan, npol, ndat)
        values["nbit%d" % nbit], read_bytes["nbit%d" % nbit] = nvalue, nbit / 8.0
    skewed = fill(nvalue, 1)
    assert skewed.data_ptr() % 2 == 1
    calls["nbit8_byte_loads"] = lambda: dspsr_amd.unpack_sigproc_fpt(ctx, skewed, rows, 8, nchan, npol, ndat)
    values["nbit8_byte_loads"], read_bytes["nbit8_byte_loads"] = nvalue, 1.0
    # the yardstick: the same number of output floats, 16-byte aligned runs
    gchan, gpol, gdat = 64, 2, nvalue // (64 * 2 * 2)
    grows = rows.view(-1)[:gchan * gpol * 2 * gdat].view(gchan, gpol, 2 * gdat)
    cs = gdat * 2 * gpol
    glay = dspsr_amd.GuppiLayout(gchan, gpol, gdat, 0, cs, gchan * cs)
    graw = fill(gchan * cs).view(torch.int8)
    calls["guppi"] = lambda: dspsr_amd.unpack_guppi_fpt(ctx, graw, grows, glay, gdat)
    values["guppi"], read_bytes["guppi"] = gchan * gpol * 2 * gdat, 1.0

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
    res = {"nchan": nchan, "npol": npol, "ndat": ndat, "windows": a.windows, "calls": a.calls, "build_id": dspsr_amd.build_id()}
    for name in calls:
        best, med, worst = min(t[name]), sorted(t[name])[len(t[name]) // 2], max(t[name])
        nbytes = (read_bytes[name] + 4.0) * values[name]
        res[name] = {"values": values[name], "model_bytes": nbytes, "best_s": best, "median_s": med, "worst_s": worst,
                     "GB_per_s_median": nbytes / med / 1e9, "GB_per_s_best": nbytes / best / 1e9, "GB_per_s_worst": nbytes / worst / 1e9,
                     "Gvalues_per_s_median": values[name] / med / 1e9}
    for name in calls:
        res[name]["time_over_guppi_median"] = res[name]["median_s"] / res["guppi"]["median_s"]
    ctx.close()
    if a.file_mib:
        res["file"] = fold_file_times(a, torch, np)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def fold_file_times(a, torch, np):
    """an 8-bit file of --file-mib MiB, 4096 channels: fold_file with -K, three times (the first includes the first launches), and
    the host read of the file's bytes (np.fromfile, the page cache warm after the write) beside it"""
    from dspsr_amd import dada, pipeline
    nchan = 4096
    ndat = (a.file_mib << 20) // nchan
    path = os.path.join(a.dir, "sigproc_unpack_probe.fil")
    rng = np.random.default_rng(2)
    with open(path, "wb") as f:
        pipeline.write_sigproc_header(f, source_name="noise", fch1=1500.0, foff=-400.0 / nchan, nchans=nchan, nbits=8, tstart_mjd=56000.0,
                                      tsamp=64e-6, nifs=1)
        f.write(rng.integers(0, 256, ndat * nchan, dtype=np.uint8).tobytes())
    out = {"bytes": os.path.getsize(path), "nchan": nchan, "ndat": ndat}
    reads = []
    for _ in range(3):
        t0 = time.perf_counter()
        np.fromfile(path, np.uint8)
        reads.append(time.perf_counter() - t0)
    out["host_read_s"] = reads
    cfg = pipeline.Config(nchan=nchan, dispersion_measure=10.0, nbin=256, folding_period=0.0123, interchan_dedispersion=True, parts_per_block=4096)
    walls, optime = [], None
    for k in range(4):
        t0 = time.perf_counter()
        lt = dada.fold_file(path, cfg if k < 3 else pipeline.Config(**dict(cfg.__dict__, record_time=True)), device=0,
                            stream=torch.cuda.current_stream().cuda_stream)
        if k < 3:
            walls.append(time.perf_counter() - t0)
        else:
            optime = {name: v[0] for name, v in lt.optime.items()}
        out["sd_head"] = lt.sd.head
        lt.close()
    out["fold_file_wall_s"] = walls
    out["record_time_s"] = optime                                    # -r: every operation ends with a stream synchronisation
    os.remove(path)
    return out


if __name__ == "__main__":
    main()
