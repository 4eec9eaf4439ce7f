"""One small run of every path through the pipeline drivers, public API only: the host arithmetic each one leaves behind.
usage: python tools/pipeline_paths.py [--record FILE.json] [--dump DIR] [--case NAME ...]

Every fold case builds its driver with parts_per_block 3, feeds three blocks of seeded int8 noise with record_time on, and calls
finish_subint; every search case feeds the calls listed with it (parts, or time samples where there is no -F).  What comes out is a record of host numbers -- derived attributes, the counters
after each block, the books of every sub-integration, the operations timed and how often -- with floats as float.hex():
tests/test_gpu_pipeline_paths.py compares it with tests/golden/pipeline_paths.json for exact equality.  --dump DIR also writes each
case's profiles and packed bytes as .npy, for a byte comparison of two checkouts.  The geometries are those of the pipeline tests of
each path (test_gpu_plain, test_gpu_parity, test_gpu_multigpu, test_gpu_cyclic_pipeline, test_gpu_plfb_pipeline, test_gpu_fold_many,
test_gpu_fourth_moment, test_gpu_search, test_gpu_direct_search, test_gpu_tfp, test_gpu_fits_pipeline).  A LoadToFITS case records the
blocks each call completes, and dumps their bytes, DAT_SCL and DAT_OFFS."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

ATTRS = ("nkeep", "nsamp_step", "nsamp_overlap", "in_nchan", "nchan_out", "npol_out", "out_rate", "out_start", "scalefac", "sd_head",
         "fused_mode")
NBLOCKS = 3
BASE = dict(freq=1382.0, bw=-16.0, tsamp=1.0 / 32.0, dm=30.0, period=0.004, nchan=16, nbin=64)          # test_gpu_parity / test_gpu_plain


def _hex(v):
    """floats as float.hex(), numpy scalars as Python numbers: the record is compared for equality"""
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    return v


def _fold_cfg(pipeline, **kw):
    b = BASE
    args = dict(nchan=b["nchan"], dispersion_measure=b["dm"], nbin=b["nbin"], folding_period=b["period"], ndim=4, parts_per_block=3,
                max_parts=2, record_time=True)
    args.update(kw)
    return pipeline.Config(**args)


def _fold_info(pipeline, **kw):
    b = BASE
    args = dict(centre_frequency=b["freq"], bandwidth=b["bw"], tsamp_us=b["tsamp"], machine="DADA")
    args.update(kw)
    return pipeline.InputInfo(**args)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _with_boundary(pipeline, make):
    """`make(subint_seconds)` -> (cfg, info, kwargs); the sub-integration is 1.6 blocks long, so that a boundary falls inside the
    second block (the length comes from a probe of the same geometry, as test_gpu_fourth_moment does it)"""
    cfg, info, kw = make(0.0)
    probe = pipeline.LoadToFold(cfg, info, stream=_stream(), **kw)
    subint = 1.6 * cfg.parts_per_block * probe.nkeep / probe.out_rate
    probe.close()
    return make(subint)


def fold_cases(pipeline):
    """name -> () -> (cfg, info, LoadToFold keywords)"""
    P = pipeline
    e2e = dict(freq=1382.0, bw=-8.0, tsamp_us=1.0 / 16.0, dm=20.0, period=0.002, nchan=8, nbin=64, freq_res=512)     # test_gpu_fourth_moment
    two = P.InputInfo(centre_frequency=1400.0, bandwidth=-32.0, nchan=2, npol=2, ndim=2, tsamp_us=1.0 / 16.0, machine="DADA")
    targets = [P.FoldTarget("a", folding_period=0.004, nbin=64), P.FoldTarget("b", folding_period=0.00123, nbin=32, reference_phase=0.25)]
    return {
        "during_fused": lambda: (_fold_cfg(P, fused_fold=True, force_fused=True), _fold_info(P), {}),
        "during_L": lambda: _with_boundary(P, lambda s: (_fold_cfg(P, fused_fold=True, force_fused=True, subint_seconds=s), _fold_info(P), {})),
        "during_K": lambda: (_fold_cfg(P, interchan_dedispersion=True), _fold_info(P), {}),
        # (test_gpu_multigpu's -K shards, cut down to two input channels)
        "during_subband_K": lambda: (P.Config(nchan=32, dispersion_measure=3.0, nbin=128, folding_period=0.0123, freq_res=256, ndim=4,
                                              parts_per_block=3, max_parts=2, interchan_dedispersion=True, record_time=True), two,
                                     dict(subband=1)),
        "after": lambda: (_fold_cfg(P, convolve_when="after"), _fold_info(P), {}),
        "never": lambda: (_fold_cfg(P, convolve_when="never"), _fold_info(P, machine="CASPSR"), {}),
        "before": lambda: (_fold_cfg(P, convolve_when="before", freq_res=32768), _fold_info(P), {}),
        "cyclic": lambda: (_fold_cfg(P, nbin=32, cyclic_nchan=16, cyclic_mover=2, cyclic_npol=2), _fold_info(P, mjd_sec=0.0), {}),
        "plfb": lambda: (P.Config(nchan=8, dispersion_measure=3.0, nbin=64, folding_period=0.0004, parts_per_block=3, plfb_nbin=8,
                                  plfb_nchan=64, record_time=True), _fold_info(P, mjd_sec=0.0), {}),
        "two_targets_s": lambda: (_fold_cfg(P, folding_period=0.0, subint_turns=1.0), _fold_info(P), dict(targets=targets)),
        "fourth_moment": lambda: _with_boundary(P, lambda s: (
            P.Config(nchan=e2e["nchan"], dispersion_measure=e2e["dm"], nbin=e2e["nbin"], folding_period=e2e["period"], freq_res=e2e["freq_res"],
                     parts_per_block=3, max_parts=2, subint_seconds=s, fourth_moment=True, ndim=2, record_time=True),
            P.InputInfo(centre_frequency=e2e["freq"], bandwidth=e2e["bw"], tsamp_us=e2e["tsamp_us"], machine="DADA"), {})),
    }


def search_cases(pipeline):
    """name -> () -> (driver, [block lengths in the driver's units])"""
    P = pipeline
    info = P.InputInfo(centre_frequency=1382.0, bandwidth=-400.0, nchan=1, npol=2, ndim=1, tsamp_us=0.00125, machine="DADA")     # test_gpu_search
    direct = P.InputInfo(centre_frequency=1400.0, bandwidth=-8.0, nchan=8, npol=2, ndim=2, tsamp_us=1.0, machine="DADA",
                         start_seconds=0.5, mjd_day=55299, mjd_sec=7545.0)                                                     # test_gpu_direct_search
    fits_real = P.InputInfo(centre_frequency=1400.0, bandwidth=-16.0, nchan=1, npol=2, ndim=1, tsamp_us=1.0 / 32.0, machine="DADA")
    fits_direct = P.InputInfo(centre_frequency=1400.0, bandwidth=4.0, nchan=4, npol=2, ndim=2, tsamp_us=1.0, machine="DADA")
    coh = dict(nchan=64, tscrunch=16, nbit=8, rescale_seconds=2e-4, freq_res=1024, parts_per_block=3, max_parts=4)
    return {
        "coherent_fused": lambda: (P.LoadToFilCoherent(P.SearchConfig(dispersion_measure=2.0, **coh), info, stream=_stream()), [3, 3, 3]),
        # (dispersion measure 0.25: the delay across the band, about 2050 samples, fits a block of three parts)
        "coherent_K_f": lambda: (P.LoadToFilCoherent(P.SearchConfig(dispersion_measure=0.25, dedisperse=True, fscrunch=4, **coh), info,
                                                     stream=_stream()), [3, 3, 3]),
        "direct_K": lambda: (P.LoadToFilDirect(P.SearchConfig(tscrunch=4, nbit=8, rescale_seconds=256.5 * 4 / 1e6, parts_per_block=2048,
                                                              dispersion_measure=20.0, dedisperse=True), direct, stream=_stream()),
                             [2000, 300, 700]),
        "fil": lambda: (P.LoadToFil(P.SearchConfig(nchan=64, tscrunch=16, nbit=8, rescale_seconds=2e-4, parts_per_block=64), info,
                                    stream=_stream()), [64, 64, 32]),
        "coherent_d4": lambda: (P.LoadToFilCoherent(P.SearchConfig(dispersion_measure=2.0, npol=4, **coh), info, stream=_stream()), [3, 3, 2]),
        # (the `real` and `direct` shapes of test_gpu_fits_pipeline, in its unequal cuts: a call that completes no block, one that
        # completes several)
        "fits_F_D": lambda: (P.LoadToFITS(P.FitsConfig(nchan=16, convolve=True, freq_res=256, dispersion_measure=1.0, coherent_dedisp=True,
                                                       tsamp=16e-6, parts_per_block=14, npol=4, nbit=4, nsblk=128), fits_real,
                                          stream=_stream()), [1, 5, 2, 6]),
        "fits_direct_K": lambda: (P.LoadToFITS(P.FitsConfig(nchan=0, dispersion_measure=100.0, tsamp=16e-6, parts_per_block=16384, npol=2,
                                                            nbit=8, nsblk=128, dedisperse=True), fits_direct, stream=_stream()),
                                  [100, 7000, 1, 0, 5887]),
    }


def _noise(seed, n):
    return np.random.default_rng(seed).integers(-40, 41, size=n, dtype=np.int8)


def _attrs(drv):
    rec = {a: _hex(getattr(drv, a, None)) for a in ATTRS}
    rec["block_bytes"] = int(drv.block_bytes())
    return rec


def _books(subints):
    return [{"hits": [int(h) for h in s["hits"]], "integration_length": _hex(s["integration_length"]), "ndat_total": int(s["ndat_total"]),
             "keys": sorted(s)} for s in subints]


def run_fold(pipeline, name, seed):
    import torch
    cfg, info, kw = fold_cases(pipeline)[name]()
    lt = pipeline.LoadToFold(cfg, info, stream=_stream(), **kw)
    rec, arrays = {"attrs": _attrs(lt), "blocks": []}, {}
    per_sample = lt.in_nchan * info.npol * info.ndim              # bytes per input time sample (CASPSR: 2 as well)
    step = cfg.parts_per_block * lt.nsamp_step
    nbytes = max((NBLOCKS - 1) * step * per_sample + lt.block_bytes(), (NBLOCKS * step + lt.nsamp_overlap) * per_sample)
    raw = torch.from_numpy(_noise(seed, nbytes)).cuda()
    for b in range(NBLOCKS):
        lt.process_block(raw[b * step * per_sample:b * step * per_sample + lt.block_bytes()])
        rec["blocks"].append([int(lt.nsamples_in), int(lt.ndat_out)])
    lt.finish_subint()
    lt.synchronize()
    groups = [("", lt.subints)] if not lt.pulsars else [("_%s" % p.target.name, p.subints) for p in lt.pulsars]
    rec["subints"] = {tag.lstrip("_"): _books(subs) for tag, subs in groups}
    for tag, subs in groups:
        for k, s in enumerate(subs):
            arrays["%s%s_sub%d" % (name, tag, k)] = pipeline.subint_profile(s)
    rec["optime"] = {op: int(n) for op, (_t, n) in lt.optime.items()}
    lt.close()
    return rec, arrays


def run_search(pipeline, name, seed):
    import torch
    drv, blocks = search_cases(pipeline)[name]()
    rec, arrays = {"attrs": _attrs(drv), "blocks": [], "header": {k: _hex(v) for k, v in drv.header_values().items()}}, {}
    for b, n in enumerate(blocks):
        raw = torch.from_numpy(_noise(seed + b, drv.block_bytes(n))).cuda()
        packed = drv.process_block(raw, n)
        drv.synchronize()
        if isinstance(packed, list):                      # LoadToFITS: the blocks this call completed
            rec["blocks"].append([len(packed), int(drv.nblocks_out)])
            for k, blk in enumerate(packed):
                for what, t in zip(("bytes", "dat_scl", "dat_offs"), blk):
                    arrays["%s_call%d_block%d_%s" % (name, b, k, what)] = t.cpu().numpy().copy()
            continue
        rec["blocks"].append([int(packed.numel()), int(drv.ndat_out)])
        arrays["%s_block%d" % (name, b)] = packed.cpu().numpy().copy()
    drv.close()
    return rec, arrays


def case_names(pipeline):
    return list(fold_cases(pipeline)) + list(search_cases(pipeline))


def run_case(pipeline, name):
    """(record, {array name: numpy array}) of one case"""
    names = case_names(pipeline)
    seed = 1000 + 10 * names.index(name)
    return (run_fold if name in fold_cases(pipeline) else run_search)(pipeline, name, seed)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--record", metavar="FILE", help="write the records of all cases as JSON")
    ap.add_argument("--dump", metavar="DIR", help="write profiles and packed bytes as .npy")
    ap.add_argument("--case", action="append", help="run only these cases")
    args = ap.parse_args()
    from dspsr_amd import pipeline
    out = {}
    for name in args.case or case_names(pipeline):
        rec, arrays = run_case(pipeline, name)
        out[name] = rec
        print("%-18s blocks %s, %d arrays" % (name, rec["blocks"], len(arrays)), flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            for key, a in arrays.items():
                np.save(os.path.join(args.dump, key + ".npy"), a)
    if args.record:
        with open(args.record, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
