#!/usr/bin/env python3
"""tools/matrix_probe.py : what the matrix response (`dspsr -pac`, csrc/fb_inv_chan_matrix.hip) costs on the headline geometry
(-F 1024:D -x 4096, DM 1000, 32 parts per launch group, raw 8-bit real dual-polarisation input).

One process: two objects of the same geometry -- the scalar response through set_kernel with DSPSR_AMD_FUSED_NEVER (the path
perform_detect takes without this feature) and chirp x Jones through set_response_matrix -- are warmed up, then perform_detect
(Coherence, ndim 4) of one launch group is timed with device events, the two variants alternating; every alternation runs enough
calls of a variant for >= 1 s of work per variant over the run.  Prints ONE JSON line: both rates in Msamples/s (input samples
of one polarisation), their ratio, the spread over the alternations, the build id.  --out FILE also writes the line there.
A kernel trace of this script (rocprofv3 --kernel-trace --stats, in a run of its own) gives the inverse pass's own time.
Recorded, not gated."""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nchan", type=int, default=1024)
    ap.add_argument("--freq-res", type=int, default=4096)
    ap.add_argument("--dm", type=float, default=1000.0)
    ap.add_argument("--parts", type=int, default=32, help="parts per launch group (= parts per call)")
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=1.2, help="timed work per variant over the whole run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import dspsr_amd
    from dspsr_amd import pipeline, polcal

    freq, bw = 1382.0, -400.0
    resp = dspsr_amd.Dedispersion(freq, bw, a.dm)
    resp.set_frequency_resolution(a.freq_res)
    resp.match(a.nchan)
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    # a calibrator of 512 channels across the band: gains and leakages of a few per cent, a phase slope between the two receptors
    ncal = 512
    cf = freq + ((np.arange(ncal) + 0.5) / ncal - 0.5) * abs(bw)
    rng = np.random.default_rng(1)
    jones = np.empty((ncal, 2, 2), np.complex128)
    jones[:, 0, 0] = 1.0 + 0.05 * rng.standard_normal(ncal)
    jones[:, 1, 1] = (1.0 + 0.05 * rng.standard_normal(ncal)) * np.exp(1j * np.linspace(0.0, 6.0, ncal))
    jones[:, 0, 1] = 0.03 * (rng.standard_normal(ncal) + 1j * rng.standard_normal(ncal))
    jones[:, 1, 0] = 0.03 * (rng.standard_normal(ncal) + 1j * rng.standard_normal(ncal))
    obs = pipeline.InputInfo(centre_frequency=freq, bandwidth=bw)
    matrix = polcal.response_product(polcal.jones_response(cf, jones, obs, a.nchan, resp.ndat), resp.kernel)

    def engine(**kw):
        return dspsr_amd.FilterbankEngine(ctx).setup(a.nchan, resp.ndat, resp.impulse_pos, resp.impulse_neg, 1, 2, True,
                                                     max_parts=a.parts, fused_fold=dspsr_amd.FUSED_NEVER, **kw)
    engines = {"scalar": engine(kernel=resp.kernel), "matrix": engine(response_matrix=matrix)}
    e0 = engines["scalar"]
    assert (engines["scalar"].response_ndim(), engines["matrix"].response_ndim()) == (2, 8)
    nsamp = a.parts * e0.nsamp_step + e0.nsamp_overlap
    raw = torch.randint(-64, 64, (2 * nsamp,), dtype=torch.int8, device="cuda")
    det = torch.empty((a.nchan, 1, 4 * a.parts * e0.nkeep), dtype=torch.float32, device="cuda")
    scale = dspsr_amd.eight_bit_scale()

    def calls(eng, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            eng.perform_detect(det, a.parts, dspsr_amd.COHERENCE, 4, raw=raw, layout=dspsr_amd.RAW_GENERIC, scale=scale)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e-3

    per_call = {}
    for name, eng in engines.items():            # warm-up, and the length of a call
        calls(eng, 3)
        per_call[name] = calls(eng, 5) / 5
    rates = {name: [] for name in engines}
    for _ in range(a.alternations):
        for name, eng in engines.items():
            n = max(1, int(round(a.seconds / a.alternations / per_call[name])))
            t = calls(eng, n)
            rates[name].append(n * a.parts * e0.nsamp_step / t / 1e6)
    med = {name: float(np.median(v)) for name, v in rates.items()}
    line = json.dumps({
        "probe": "matrix_response", "build_id": dspsr_amd.build_id(),
        "geometry": {"nchan": a.nchan, "freq_res": resp.ndat, "dm": a.dm, "nfilt": [resp.impulse_pos, resp.impulse_neg], "parts_per_call": a.parts,
                     "input": "8-bit real dual-pol", "call": "perform_detect Coherence ndim 4"},
        "scalar_msamples_per_s": med["scalar"], "matrix_msamples_per_s": med["matrix"], "matrix_over_scalar": med["matrix"] / med["scalar"],
        "spread": {name: {"min": min(v), "max": max(v), "alternations": len(v)} for name, v in rates.items()},
        "ms_per_call": {name: 1e3 * a.parts * e0.nsamp_step / (med[name] * 1e6) for name in med},
        "npass": {name: eng.npass(True) for name, eng in engines.items()},
        "presplit": {name: eng.presplit() for name, eng in engines.items()}})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for eng in engines.values():
        eng.close()
    ctx.close()


if __name__ == "__main__":
    main()
