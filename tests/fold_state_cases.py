"""The fold of the square-law states, dspsr_amd_filterbank_perform_fold with DSPSR_AMD_INTENSITY (dspsr -d 1) and DSPSR_AMD_PPQQ
(-d 2): the cases of tests/test_gpu_fold_states.py as plain data, the host's dispatch restated, and the model of the sums.

The cases are those of tests/fused_fold_cases.py -- groups psl, seg, cap, runs, placement and grid, the same geometries, calls
and plans -- with the profile shapes "1" (npol 1 x ndim 1: Intensity) and "2x1" (npol 2 x ndim 1: the rows PP and QQ).  Not
`segsum`: four-pass objects report mode 0 for these states.  What differs from the Coherence path (csrc/filterbank.hip
fb_perform_fold_sq, dspsr_amd_filterbank_fold_is_fused_state):
  - the fused kernel is k_inv_chan<., 3 | 7, .> alone: a call that takes the two-pass path (generic 8-bit complex block,
    geometry()["passes"] == 2) runs Detection + Fold although the object reports mode 1 or 2;
  - the accumulators are scalars: NO condition on a bound profile's address, span or padding -- every placement case fuses;
  - a run's partial profile is packed [chan][npol][nbin] and k_fold_combine adds the runs in order, every bin of every run.
No torch: tests/test_fold_state_cases_host.py checks the records on a machine without a GPU."""
import functools

import numpy as np

import fused_fold_cases as fc
from fold_reference import FOLD_LONG_RUN, fused_launch_sums, fused_nseg

INTENSITY, PPQQ = 2, 3                                  # dspsr_amd/_lib.py
GROUPS = ("psl", "seg", "cap", "runs", "placement", "grid")
NPO = {"1": 1, "2x1": 2}
STATE = {"1": INTENSITY, "2x1": PPQQ}

# the placements of a bound profile, (offset floats, row padding floats): rows of nbin floats at ANY float-aligned address
PLACEMENTS = (("span4", (0, 2)), ("even", (0, 0)), ("odd", (0, 3)), ("off1", (1, 2)), ("off3-odd", (3, 1)))


def _cases():
    out, seen = [], set()
    for c in fc.CASES:
        if c["group"] not in GROUPS or c["group"] == "placement":
            continue
        key = (c["C"], c["M"], c["nfilt"], c["real"], repr(c["calls"]), c["max_parts"], c["policy"], c["input_nchan"], c["four"])
        two_pass = fc.geometry(c["C"], c["M"], c["nfilt"], c["real"], c["four"])["passes"] == 2
        # a two-pass case keeps ONE shape (its call runs Detection + Fold here); a three-pass case, once per geometry and calls, both
        profs = ({"4": "1", "2x2": "2x1"}[c["prof"]],) if two_pass else ("1", "2x1")
        if key in seen and not two_pass:
            continue
        seen.add(key)
        base = c["name"][:-len(c["prof"]) - 1] if c["name"].endswith("-" + c["prof"]) else c["name"]
        if any(o["name"].startswith(base + "-") and o["base"] != c["name"] for o in out):
            base += "-b"             # (cap-around-2x2, runs-hits-2x2: other launches than their "4" twins)
        for prof in profs:
            out.append(dict(c, name="%s-%s" % (base, prof), prof=prof, base=c["name"]))
    psl = fc.by_name("place-4-span4")
    for label, bound in PLACEMENTS:
        for prof in ("1", "2x1"):
            out.append(dict(psl, name="place-%s-%s" % (prof, label), prof=prof, bound=bound, base="place-4-span4"))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), names
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]


def by_name(name):
    return CASES[NAMES.index(name)]


def of_group(group):
    return [c["name"] for c in CASES if c["group"] == group]


def call_runs(name, k):
    """(runs, per-bin hits, samples) of call k: the base case's plan"""
    return fc.call_runs(by_name(name)["base"], k)


def shape(c):
    """(nchan, npol, nbin, ndim) of the profile"""
    return c["input_nchan"] * c["C"], NPO[c["prof"]], c["nbin"], 1


def fold_mode_state(g, policy, ncu):
    """dspsr_amd_filterbank_fold_is_fused_state for INTENSITY / PPQQ (two polarisations): the Coherence mode, never 3"""
    mode = fc.fold_mode(g, policy, ncu)
    return mode if mode in (1, 2) else 0


@functools.lru_cache(maxsize=None)
def record(name, ncu=256, wg3=None):
    """What the case reaches: the mode, and per call the path ("fused" | "detect+fold"), the stand-alone fold's association
    ("time" | "long") and the fused launches (ns, nseg)."""
    c = by_name(name)
    g = fc.geometry(c["C"], c["M"], c["nfilt"], c["real"], c["four"])
    mode = fold_mode_state(g, c["policy"], ncu)
    rec = dict(mode=mode, passes=g["passes"], tiles=g["tiles"], calls=[])
    wgs = ncu * (g["wg3"] if wg3 is None else wg3) if g["passes"] == 3 else ncu
    for k, (parts, _plan) in enumerate(c["calls"]):
        runs, _hits, _ndat = call_runs(name, k)
        max_run = int(runs[:, 2].max()) if len(runs) else 0
        call = dict(max_run=max_run, launches=[])
        if mode in (1, 2) and g["passes"] == 3 and max_run < fc.FOLD_FUSED_MAX_RUN:
            call.update(path="fused", assoc=None)
            for ns in fc.launches_of(parts, c["max_parts"]):
                call["launches"].append(dict(ns=ns, nseg=fused_nseg(ns, g["tiles"], wgs) if mode == 2 else 1))
        else:
            # (the stand-alone fold reads the object's own detected rows, 16-byte aligned: runs of FOLD_LONG_RUN take the long-run kernel)
            call.update(path="detect+fold", assoc="long" if max_run >= FOLD_LONG_RUN else "time")
        rec["calls"].append(call)
    return rec


def fused_fold_model_sq(det, runs, profile, nkeep, launches, mode, nseg_of=None):
    """fold_reference.fused_fold_model for a square-law state.  det: float32 [chan][npol][ndat], the rows of perform_detect;
    profile: [chan][npol][nbin][1].  The rows of a channel are independent sums in the same order: they ride as the last axis."""
    det = np.asarray(det, np.float32)
    rows = np.ascontiguousarray(det.transpose(0, 2, 1))[:, None]                               # [chan][1][ndat][npol]
    out = np.ascontiguousarray(np.asarray(profile, np.float32)[..., 0].transpose(0, 2, 1))[:, None]    # [chan][1][nbin][npol]
    assert mode in (1, 2)
    part0 = 0
    for ns in launches:
        out, partial = fused_launch_sums(rows, runs, out, nkeep, part0, ns, 1 if mode == 1 else nseg_of(ns))
        for p in partial:
            out = out + p
        part0 += ns
    assert part0 * nkeep == det.shape[2], "the launches do not cover the call"
    return np.ascontiguousarray(out[:, 0].transpose(0, 2, 1))[..., None]


def loadtofold_block_model_sq(lt, raw, npart, profile, ncu):
    """fused_fold_cases.loadtofold_block_model for a pipeline.LoadToFold with npol 1 or 2: (mode, hits, model) of the block it is
    about to fold as ONE fused call; the model is None where the call does not take the fused kernel.  Call it BEFORE
    process_block.  (Needs torch and a device.)"""
    import torch
    import dspsr_amd
    from fold_reference import runs_of_plan
    ndat, nbin, npo = npart * lt.nkeep, lt.cfg.nbin, lt.npol_out
    phi, pfold = lt._phase(lt.out_start + (lt.ndat_out + 0.5) / lt.out_rate)
    plan, hits = dspsr_amd.fold_binplan(phi, (1.0 / lt.out_rate) / pfold, nbin, ndat)
    det = torch.zeros((lt.nchan_out, npo, ndat), dtype=torch.float32, device=raw.device)
    lt.fb.perform_detect(det, npart, lt.detection_state(), 1, raw=raw, layout=lt.layout, scale=lt.scale8)
    cfg = lt.fb.cfg
    g = fc.geometry(cfg.nchan_subband, cfg.freq_res, (cfg.nfilt_pos, cfg.nfilt_neg), bool(cfg.real_input), cfg.force_four_pass)
    mode = fold_mode_state(g, cfg.fused_fold, ncu)
    runs = runs_of_plan(plan.astype(np.int64))
    if mode not in (1, 2) or g["passes"] != 3 or (len(runs) and int(runs[:, 2].max()) >= fc.FOLD_FUSED_MAX_RUN):
        return mode, hits, None
    wgs = ncu * g["wg3"]
    model = fused_fold_model_sq(det.cpu().numpy(), runs, profile, g["nkeep"], fc.launches_of(npart, cfg.max_parts), mode,
                                lambda ns: fused_nseg(ns, g["tiles"], wgs))
    return mode, hits, model
