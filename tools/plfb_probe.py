#!/usr/bin/env python3
"""tools/plfb_probe.py : time the phase-locked filterbank (csrc/plfb.hip) with HIP events on dual-polarisation complex rows of 16
channels at 25 MHz each (a 400 MHz band through -F 16:D) for
  -F 16:D -G 256, Vela period (0.0893 s)   8192 channels per window
  -F 16:D -G 64,  period 1.6 ms            512 channels per window
npol_out 4, windows from pipeline.PlfbPlan, and append to profiles/plfb.txt, with the library's build id: time per accumulate
call and input GB/s (the bytes of the windows, each read once, over the call time), beside them FoldEngine.fold of the SAME rows
as npol 2 x ndim 2 samples into the same number of bins for scale (the engine picks k_fold_dense or k_fold_chunked by its plan),
the VGPRs and LDS of the kernels launched, and the two error figures of the noise test (tests/test_gpu_plfb.py) per nchan.
The events bracket the whole CALL: the host's sort of the windows and the upload of the plan come before the launch inside
dspsr_amd_plfb_accumulate; kernel-only times are in a kernel trace of this script (rocprofv3 --kernel-trace --stats).
Recorded, not gated."""
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kernel_resources(names):
    """{name: (vgprs, scratch bytes)} from the code objects of the shipped library"""
    import test_kernel_resources as tkr
    ks = {}
    for co in tkr._code_objects(open(tkr.LIB, "rb").read()):
        ks.update(tkr._kernels(co))
    mangled = sorted(ks)
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.splitlines()
    table = {d.split("(")[0].replace("void dspsr_amd::", "").replace("dspsr_amd::", ""): ks[m] for d, m in zip(dem, mangled)}
    return {n: (int(table[n].get(".vgpr_count", -1)), int(table[n].get(".private_segment_fixed_size", 0))) for n in names}


def lds_bytes(logc):
    """dynamic LDS of k_plfb<logc, ., .>: wgfft.h lds_total_words_host(16384, logc) complex words"""
    nq, rem = logc // 4, logc % 4
    ntw = nq - (0 if rem else 1)
    ltw = sum(4 << (logc - 4 * (st + 1)) for st in range(max(ntw, 0)))
    return 8 * (16384 + (16384 >> 6 << 2) + 8 + ltw + 8 + 16)


def main():
    import math
    import numpy as np
    import torch
    import dspsr_amd
    from dspsr_amd import pipeline
    import plfb_cases
    out = os.environ.get("PLFB_PROBE_OUT", os.path.join(ROOT, "profiles", "plfb.txt"))
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    lines = ["plfb_probe build_id=%s" % dspsr_amd.build_id()]
    nchan_in, rate, ndat = 16, 400e6 / 16, 1 << 22
    rows = torch.randn((nchan_in, 2, 2 * ndat), dtype=torch.float32, device="cuda") * 30.0
    for name, period, nbin in [("-F 16:D -G 256 (Vela)", 0.0893, 256), ("-F 16:D -G 64 (1.6 ms)", 0.0016, 64)]:
        nchan = pipeline.plfb_choose_nchan(period, rate, nbin)
        phase = lambda t: (int(math.floor(t / period)), t / period - math.floor(t / period))
        iphase = lambda ph, guess: (ph[0] + ph[1]) * period
        div = pipeline.TurnsDivider(phase, iphase, period, 0.0, rate, 1.0 / nbin, 0.0)
        starts, bins = pipeline.PlfbPlan(div, nbin, 0.0, nchan).take(ndat)
        eng = dspsr_amd.PhaseLockedFilterbankEngine(ctx)
        eng.set_shape(nchan_in, 2, 2, nchan, 4, nbin)
        fold = dspsr_amd.FoldEngine(ctx)
        fold.set_shape(nchan_in, 2, 2, nbin)
        fold.set_nbin(nbin)

        def timed(call):
            times = []
            for it in range(2 + 5):                          # two warm-up calls, then five timed ones
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                if it >= 2:
                    times.append(e0.elapsed_time(e1) * 1e-3)
            return float(np.median(times)), min(times), max(times)

        def fold_call():
            fold.set_ndat(ndat, 0)
            fold.set_bins(0.1, (1.0 / rate) / period, ndat, 0)
            fold.fold(rows)
        t, lo, hi = timed(lambda: eng.accumulate(rows, ndat, starts, bins))
        tf, flo, fhi = timed(fold_call)
        logc = int(math.log2(nchan))
        kname = "k_plfb<%d, 2, 4>" % logc
        vg, scratch = kernel_resources([kname])[kname]
        gbytes = len(starts) * nchan * 8.0 * 2 * nchan_in / 1e9
        lines.append("%s: nchan_in=%d npol 2->4 nchan=%d nbin=%d ndat=%d windows=%d (%.1f %% of the rows)  accumulate call incl. host "
                     "plan sort and upload: median %.3f ms (min %.3f max %.3f, n=5)  %.1f GB/s of window bytes;  FoldEngine.fold of the same "
                     "rows (npol 2 x ndim 2, %d bins, plan build and upload included): median %.3f ms (min %.3f max %.3f)  %.1f GB/s of row "
                     "bytes;  %s: %d VGPRs, %d bytes scratch, %d bytes LDS (dynamic)"
                     % (name, nchan_in, nchan, nbin, ndat, len(starts), 100.0 * len(starts) * nchan / ndat, t * 1e3, lo * 1e3, hi * 1e3,
                        gbytes / t, nbin, tf * 1e3, flo * 1e3, fhi * 1e3, nchan_in * 2 * ndat * 8.0 / 1e9 / tf, kname, vg, scratch,
                        lds_bytes(logc)))
        eng.close()
        fold.close()
    del rows
    vg, scratch = kernel_resources(["k_plfb_combine"])["k_plfb_combine"]
    lines.append("k_plfb_combine: %d VGPRs, %d bytes scratch, no LDS" % (vg, scratch))
    # the noise test's figures: e = max |profile - float64 reference| / max |float64 reference|, GPU and float32 strict order
    for ndim, nchan in plfb_cases.NOISE:
        r, starts, bins, ref, n, e_f32 = plfb_cases.noise_case(ndim, nchan)
        eng = dspsr_amd.PhaseLockedFilterbankEngine(ctx)
        eng.set_shape(2, 2, ndim, nchan, 4, 5)
        eng.accumulate(torch.from_numpy(r).cuda(), n, starts, bins)
        e_gpu = float(np.abs(eng.synch().astype(np.float64) - ref).max() / np.abs(ref).max())
        eng.close()
        lines.append("noise ndim=%d nchan=%d: e(GPU) %.3e  e(F32 strict order) %.3e  ratio %.2f (bound 4)" % (ndim, nchan, e_gpu, e_f32, e_gpu / e_f32))
    ctx.close()
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
