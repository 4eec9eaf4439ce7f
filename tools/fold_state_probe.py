"""perform_fold on a resident 8-bit block at the headline geometry (-F 1024:D -x 4096, nkeep 3252), for the detection
states Coherence, Intensity (dspsr -d 1) and PPQQ (-d 2), each fused (DSPSR_AMD_FUSED_AUTO) and as Detection + Fold
(DSPSR_AMD_FUSED_NEVER).  The six forms alternate inside one process on one device: ROUNDS rounds, each timing every form once over
REPS calls between two HIP events, so that drift of the device hits all forms alike.  Prints the library's build id, then per form
the median, minimum and maximum of the rounds in ms per call of PARTS parts: the yardstick is the Coherence time of the same run,
the margin the spread of its own rounds.
  python tools/fold_state_probe.py [parts [rounds [reps [nchan [always]]]]]     (always: DSPSR_AMD_FUSED_ALWAYS as the fused form -- fewer than 8 tiles)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dspsr_amd  # noqa: E402


def main():
    parts, rounds, reps, C = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 32), (2, 7), (3, 5), (4, 1024)))
    M, nfilt, nbin = 4096, (422, 422), 1024
    nkeep = M - sum(nfilt)
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    print("build", dspsr_amd.build_id(), "nchan %d freq_res %d nkeep %d parts %d rounds %d reps %d" % (C, M, nkeep, parts, rounds, reps))
    nsamp = 2 * C * (parts * nkeep + sum(nfilt))
    raw = torch.randint(-100, 100, (2 * nsamp,), dtype=torch.int8, device="cuda")
    kernel = np.exp(1j * np.random.default_rng(1).uniform(-np.pi, np.pi, C * M)).astype(np.complex64)
    ndat = parts * nkeep
    pps = 1.0 / (nbin * 34.0)                             # the headline's 34-sample runs
    forms = []
    for sname, state, shape in (("Coherence", dspsr_amd.COHERENCE, (1, 4)), ("Intensity", dspsr_amd.INTENSITY, (1, 1)), ("PPQQ", dspsr_amd.PPQQ, (2, 1))):
        for pname, policy in (("fused", dspsr_amd.FUSED_ALWAYS if "always" in sys.argv[5:] else dspsr_amd.FUSED_AUTO), ("unfused", dspsr_amd.FUSED_NEVER)):
            eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, nfilt[0], nfilt[1], 1, 2, True, kernel, max_parts=32, fused_fold=policy)
            fold = dspsr_amd.FoldEngine(ctx)
            fold.set_shape(C, shape[0], shape[1], nbin)
            forms.append(("%s %s (mode %d)" % (sname, pname, eng.fold_is_fused(state)), eng, fold, state, []))

    def call(eng, fold, state):
        fold.set_nbin(nbin)
        fold.set_ndat(ndat, 0)
        fold.set_bins(0.1, pps, ndat, 0, None)
        eng.perform_fold(fold, parts, state, raw=raw, scale=1.0)

    for _name, eng, fold, state, _t in forms:                # warm-up: allocations, plans
        call(eng, fold, state)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for _name, eng, fold, state, times in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _r in range(reps):
                call(eng, fold, state)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / reps)
    for name, eng, fold, _state, times in forms:
        t = np.sort(np.array(times))
        print("%-28s median %8.3f ms  min %8.3f  max %8.3f   %9.0f Msamples/s" % (name, np.median(t), t[0], t[-1], nsamp / np.median(t) / 1e3))
        eng.close()
        fold.close()
    ctx.close()


if __name__ == "__main__":
    main()
