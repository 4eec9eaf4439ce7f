"""Search mode with the four Coherence products on a resident 8-bit block: perform_search(COHERENCE) -- detection and time scrunch
inside the inverse pass where the staged tile fits -- against the route it replaces, perform_detect(COHERENCE, ndim 1) followed by
tscrunch_fpt (npol 4), both on the SAME object and block.  Two shapes, 400 MHz of 8-bit real dual-polarisation input at 1382 MHz:

  digifits   -F 4096:D -D 1000 -do_dedisp true -t 64e-6 -p 4      tres_factor 6; the response chooses freq_res 512, nkeep 458
  digifil    -F 1024:D -x 4096 -D 1000 -t 16 -d 4                 the headline's filterbank, nkeep 3252

whose geometry comes from the drivers' own host plans.  One process, one device; a warm-up call of each route (allocations), then
ROUNDS rounds in which the two routes alternate, each timed over REPS calls between two HIP events, REPS chosen so that a window
lasts about WINDOW seconds.  Prints the library's build id and, per shape and route, median, minimum and maximum of the rounds in
ms per call of PARTS parts, and the ratio of the medians.
  python tools/coherence_search_probe.py [parts [rounds [window_seconds]]]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dspsr_amd  # noqa: E402
from dspsr_amd import pipeline  # noqa: E402

INFO = dict(centre_frequency=1382.0, bandwidth=-400.0, nchan=1, npol=2, ndim=1, tsamp_us=0.00125, machine="DADA")


def shapes():
    """(name, nchan, response, scrunch factor) from the host plans of the two drivers"""
    info = pipeline.InputInfo(**INFO)
    lt = pipeline.LoadToFITS(pipeline.FitsConfig(nchan=4096, convolve=True, dispersion_measure=1000.0, coherent_dedisp=True, tsamp=64e-6, npol=4,
                                                 nbit=2), info, device=None)
    lf = pipeline.LoadToFilCoherent(pipeline.SearchConfig(nchan=1024, tscrunch=16, nbit=8, dispersion_measure=1000.0, freq_res=4096, npol=4),
                                    info, device=None)
    return [("digifits -F 4096:D -t 64e-6 -p 4", 4096, lt.front.response, lt.tres_factor),
            ("digifil -F 1024:D -x 4096 -t 16 -d 4", 1024, lf.front.response, 16)]


def main():
    parts, rounds = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 32), (2, 5)))
    window = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    print("build", dspsr_amd.build_id(), "device", torch.cuda.get_device_name(0), "parts %d rounds %d window %.2f s" % (parts, rounds, window))
    for name, C, r, sf in shapes():
        fb = dspsr_amd.FilterbankEngine(ctx).setup(C, r.ndat, r.impulse_pos, r.impulse_neg, 1, 2, True, r.kernel, max_parts=32)
        nkeep, ndat = fb.nkeep, parts * fb.nkeep
        fused = fb.search_fuses(dspsr_amd.COHERENCE, sf)
        raw = torch.randint(-100, 100, (2 * (parts * fb.nsamp_step + fb.nsamp_overlap),), dtype=torch.int8, device="cuda")
        nout = ndat // sf + 1
        out = torch.zeros((C, 4, nout), dtype=torch.float32, device="cuda")
        out2 = torch.zeros((C, 4, nout), dtype=torch.float32, device="cuda")
        det = torch.zeros((C, 4, ndat), dtype=torch.float32, device="cuda")
        carry = torch.zeros((C, 4), dtype=torch.float32, device="cuda")
        carry2 = torch.zeros((C, 4), dtype=torch.float32, device="cuda")
        block = dict(raw=raw, layout=dspsr_amd.RAW_GENERIC, scale=1.0)

        def search():
            return fb.perform_search(out, carry, 0, parts, sf, dspsr_amd.COHERENCE, **block)

        def unfused():
            fb.perform_detect(det, parts, dspsr_amd.COHERENCE, 1, **block)
            return pipeline.tscrunch_fpt(ctx, det, out2, sf, carry2, 0)

        routes = [("perform_search(COHERENCE)%s" % ("" if fused else " [NOT fused here]"), search, []), ("perform_detect + tscrunch_fpt", unfused, [])]

        def timed(fn, reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps

        got = [fn() for _n, fn, _t in routes]              # warm-up: allocations
        torch.cuda.synchronize()
        # (the carries are compared only where the call leaves samples in them: their content is undefined at a count of 0)
        same = got[0] == got[1] and torch.equal(out[:, :, :got[0][0]], out2[:, :, :got[0][0]]) and (got[0][1] == 0 or torch.equal(carry, carry2))
        reps = [max(1, int(window * 1e3 / max(timed(fn, 3), 1e-3))) for _n, fn, _t in routes]
        for _ in range(rounds):
            for (_n, fn, times), n in zip(routes, reps):
                times.append(timed(fn, n))
        print("%s: nchan %d freq_res %d nkeep %d tscrunch %d, G %d, tscrunch * G = %d; %d samples per call; the two routes give %s" % (
            name, C, r.ndat, nkeep, sf, ((nkeep + 2 * sf - 2) // sf) | 1, sf * (((nkeep + 2 * sf - 2) // sf) | 1), ndat,
            "the same bits" if same else "DIFFERENT results"))
        med = []
        for (rname, _fn, times), n in zip(routes, reps):
            t = np.sort(np.array(times))
            med.append(float(np.median(t)))
            print("  %-44s %4d calls per window  median %8.3f ms  min %8.3f  max %8.3f   %8.0f Msamples/s of input" % (
                rname, n, med[-1], t[0], t[-1], raw.numel() / 2 / med[-1] / 1e3))
        print("  fused / unfused = %.3f" % (med[0] / med[1]))
        fb.close()
        del raw, out, out2, det
    ctx.close()


if __name__ == "__main__":
    main()
