#!/usr/bin/env python3
"""tools/cyclic_probe.py : time the cyclic-fold kernel group (csrc/cyclic_fold.hip) with HIP events on dual-polarisation rows for
  -F 64:D -cyclic 256                       (64 channels, nlag 129)
  -F 1:D  -cyclic 1024 -cyclicoversample 4  (1 channel, nlag 2049)
npol_out 4, and append samples/s, achieved fp32 FLOP/s (8 flops per complex multiply-add, nlag * npol_out of them per sample and
channel) and the fraction of the vector fp32 peak to profiles/cyclic_fold.txt with the library's build id.  Recorded, not gated.
The events bracket the whole fold CALL: the host's run-list build and its upload come before the launch inside
dspsr_amd_cyclic_fold_fold, so the figure is that of the call, not of the kernels alone -- those are in the kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/cyclic_probe.py).  After the timing, one fold of the same rows is compared on a
slice (channel 0, four lags, products p0p0 and p0p1) with float64 and with float32 sums in strict time order: e(GPU), e(F32)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
PEAK_FP32 = 157.3e12      # MI355X vector fp32, FLOP/s (256 CUs x 128 FMA lanes x 2 x 2.4 GHz)


def slice_errors(np, eng, rows, nlag, ndat, nbin, pps):
    """max over the slice of e(X) = max |X - R64| / max |R64| per lag function, for X = the device's sums and X = float32 sums in
    strict time order (each term two rounded products and a rounded sum, as the CPU loop forms it)"""
    import dspsr_amd
    eng.zero()
    eng.set_ndat(ndat, 0)
    eng.set_bins(0.1, pps, ndat, 0)
    eng.fold(rows)
    got = eng.synch_lags()                                   # [bin][pol][chan][lag][2]
    p0, p1, _ = dspsr_amd.cyclic_binplan(0.1, pps, nbin, ndat)
    x = rows[0].cpu().numpy().reshape(2, ndat, 2)
    n = ndat - nlag
    lags = [0, 1, nlag // 2, nlag - 1]
    worst = [0.0, 0.0]
    for q, py in ((0, 0), (2, 1)):                           # p0 conj(p0), p0 conj(p1)
        r64 = np.zeros((nbin, len(lags)), np.complex128)
        f32 = np.zeros((nbin, len(lags)), np.complex64)
        for k, l in enumerate(lags):
            a, b = x[0, :n], x[py, l:l + n]
            bins = (p1 if l % 2 else p0)[l // 2:l // 2 + n]
            tr = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]       # float32 arithmetic: rounded products, rounded sum
            ti = a[:, 1] * b[:, 0] - a[:, 0] * b[:, 1]
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            r64[:, k] = (np.bincount(bins, a64[:, 0] * b64[:, 0] + a64[:, 1] * b64[:, 1], nbin)
                         + 1j * np.bincount(bins, a64[:, 1] * b64[:, 0] - a64[:, 0] * b64[:, 1], nbin))
            order = np.argsort(bins, kind="stable")          # time order within every bin
            ends = np.cumsum(np.bincount(bins, minlength=nbin))
            start = 0
            for ib, end in enumerate(ends):
                if end > start:                              # cumsum of float32 adds one term at a time, in order
                    f32[ib, k] = np.cumsum(tr[order[start:end]], dtype=np.float32)[-1] + 1j * np.cumsum(ti[order[start:end]], dtype=np.float32)[-1]
                start = end
        g = got[:, q, 0, lags, 0] + 1j * got[:, q, 0, lags, 1]
        peak = np.abs(r64).max()
        worst[0] = max(worst[0], float(np.abs(g - r64).max() / peak))
        worst[1] = max(worst[1], float(np.abs(f32 - r64).max() / peak))
    return worst


def main():
    import numpy as np
    import torch
    import dspsr_amd
    out = os.environ.get("CYCLIC_PROBE_OUT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "cyclic_fold.txt"))
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    lines = ["cyclic_probe build_id=%s" % dspsr_amd.build_id()]
    for name, nchan, nlag, mover, ndat, nbin, pps in [("-F 64:D -cyclic 256", 64, 129, 1, 1 << 18, 256, 1.0 / 256 / 12.5),
                                                       ("-F 1:D -cyclic 1024 -cyclicoversample 4", 1, 2049, 4, 1 << 20, 256, 1.0 / 256 / 800.0)]:
        rows = torch.randn((nchan, 2, 2 * ndat), dtype=torch.float32, device="cuda") * 30.0
        eng = dspsr_amd.CyclicFoldEngine(ctx)
        eng.set_shape(nchan, 2, 4, nlag, mover, nbin)
        times = []
        for it in range(2 + 5):                               # two warm-up calls, then five timed ones
            eng.set_ndat(ndat, 0)
            eng.set_bins(0.1, pps, ndat, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.fold(rows)
            eng.get_lagdata_ptr()                             # the combine of the partial arrays belongs to the group
            e1.record()
            e1.synchronize()
            if it >= 2:
                times.append(e0.elapsed_time(e1) * 1e-3)
        t = float(np.median(times))
        e_gpu, e_f32 = slice_errors(np, eng, rows, nlag, ndat, nbin, pps)
        flops = 8.0 * nlag * 4 * nchan * (ndat - nlag)
        lines.append("%s: nchan=%d nlag=%d npol_out=4 nbin=%d ndat=%d  fold call incl. host run-list build and upload: median %.3f ms "
                     "(min %.3f max %.3f, n=5)  %.4g samples/s  %.4g fp32 FLOP/s  %.1f %% of the vector fp32 peak;  slice errors against "
                     "float64: e(GPU) %.3g  e(F32 strict order) %.3g" % (name, nchan, nlag, nbin, ndat, t * 1e3, min(times) * 1e3, max(times) * 1e3,
                                                                         nchan * ndat / t, flops / t, 100 * flops / t / PEAK_FP32, e_gpu, e_f32))
        eng.close()
    ctx.close()
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
