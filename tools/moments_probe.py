#!/usr/bin/env python3
"""tools/moments_probe.py : the three ways to fold a block of Stokes rows at the headline's detected shape (1024 channels, nbin
1024, one block of 64 parts of 3252 samples, 34-sample runs: the exact time-order kernels)

  1  fold4     the ndim 4 fold of the Stokes rows (dspsr_amd_fold_fold into npol 1 x ndim 4: what a run without -4 does)
  2  stream    dspsr_amd_fourth_moment, then dspsr_amd_fold_fold of the ndim 14 stream it wrote (the reference's way)
  3  moments   dspsr_amd_fold_fold_moments of the Stokes rows (the products formed in registers)

alternating, with HIP events around each CALL (the host's plan build and upload included; the plan itself is set before the
first event), and appends the medians, the bytes each variant must move per sample and the library's build id to
profiles/fourth_moment.txt.  Kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o moments -- python tools/moments_probe.py
whose <DIR>/*kernel_stats.csv lists k_fold_dense<4, 1>, k_fourth_moment and k_fold_moments<...> by name.  Recorded, not gated.
Variants 2 and 3 are compared bit for bit before anything is written."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NCHAN, NBIN, NDAT, PERIOD = 1024, 1024, 64 * 3252, 34816.0
# bytes per sample and channel that must cross HBM: the Stokes float4 | the float4 read, 14 floats written, 14 floats read
BYTES = {"fold4": 16, "stream": 16 + 56 + 56, "moments": 16}


def main():
    import numpy as np
    import torch
    import dspsr_amd
    out = os.environ.get("MOMENTS_PROBE_OUT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "fourth_moment.txt"))
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    stokes = torch.randn((NCHAN, 1, 4 * NDAT), dtype=torch.float32, device="cuda")
    stream = torch.empty((NCHAN, 1, 14 * NDAT), dtype=torch.float32, device="cuda")
    e4, es, em = (dspsr_amd.FoldEngine(ctx) for _ in range(3))
    e4.set_shape(NCHAN, 1, 4, NBIN)
    es.set_shape(NCHAN, 1, 14, NBIN)
    em.set_shape(NCHAN, 1, 14, NBIN)

    def plan(eng):
        eng.set_nbin(NBIN)
        eng.set_ndat(NDAT, 0)
        eng.set_bins(0.1, 1.0 / PERIOD, NDAT, 0)

    def stream_call():
        dspsr_amd.fourth_moment(ctx, stokes, stream)
        es.fold(stream)
    variants = [("fold4", e4, lambda: e4.fold(stokes)), ("stream", es, stream_call), ("moments", em, lambda: em.fold_moments(stokes))]
    times = {name: [] for name, _, _ in variants}
    for it in range(2 + 7):                                    # two warm-up rounds, then seven timed ones, the variants alternating
        for name, eng, call in variants:
            plan(eng)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if it >= 2:
                times[name].append(e0.elapsed_time(e1) * 1e-3)
    for eng in (es, em):                                       # one fold each into a zero profile: the same bits
        eng.zero()
        plan(eng)
    stream_call()
    em.fold_moments(stokes)
    same = bool(np.array_equal(es.synch().view(np.uint32), em.synch().view(np.uint32)))
    lines = ["moments_probe build_id=%s nchan=%d nbin=%d ndat=%d period=%g samples  stream == moments bit for bit: %s"
             % (dspsr_amd.build_id(), NCHAN, NBIN, NDAT, PERIOD, same)]
    for name, _, _ in variants:
        t = float(np.median(times[name]))
        nbytes = BYTES[name] * NCHAN * NDAT
        lines.append("  %-8s call: median %.3f ms (min %.3f max %.3f, n=%d)  %d bytes per sample, %.3f GB per block, %.0f GB/s of them"
                     % (name, t * 1e3, min(times[name]) * 1e3, max(times[name]) * 1e3, len(times[name]), BYTES[name], nbytes * 1e-9,
                        nbytes * 1e-9 / t))
    for eng in (e4, es, em):
        eng.close()
    ctx.close()
    if not same:
        sys.exit("\n".join(lines) + "\nthe two loaders disagree: nothing recorded")
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
