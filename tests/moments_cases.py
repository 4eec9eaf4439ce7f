"""Fourth-order moments (`dspsr -4`) for the tests: the numpy restatement of dsp::FourthMoment::transformation, the launch
arithmetic of the moments fold (csrc/fold_moments.hip fold_moments_run) and the table of cases tests/test_gpu_fourth_moment.py
folds, each with the edge it is there for (tests/test_moments_host.py shows, without a GPU, that it reaches it).

The sums themselves need no model of their own: a fold of npol 1 x ndim 14 rows is the fold of tests/fold_reference.py at ndim
14 -- fold_time_order for plans of short runs, and for plans with a run of FOLD_LONG_RUN samples or more fold_long_model with
nrow = nchan * ngroup: the kernel cuts the row into the same time segments of whole 2048-sample units and sums runs around the
same 32-sample micro-blocks; its own chunk (2048 samples of ndim 4, 512 of ndim 14) only cuts runs at micro-block boundaries,
which leaves the sequence of additions as it is.
"""
import os

import numpy as np

from fold_reference import FOLD_CHUNK, FOLD_LONG_RUN, FOLD_MB, long_segments, plan_span, runs_of_plan

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dspsr_amd", "csrc", "fold_moments.hip")

MOM_NDIM = 14
MOM_THREADS = 256
MOM_BPT = 2
MOM_MB = 32
MOM_SEG_UNIT = 2048
MOM_CHUNK_STOKES = 2048
MOM_CHUNK_STREAM = 512
MOM_FM_SAMPLES = 256
NCU_MI355X = 256

# FourthMoment.C:67-72: for (i = 0; i < 4; i++) for (j = i; j < 4; j++) *out++ = in[i] * in[j]
PAIRS = []
for _i in range(4):
    for _j in range(_i, 4):
        PAIRS.append((_i, _j))
PAIRS = tuple(PAIRS)


def fourth_moment(stokes):
    """dsp::FourthMoment::transformation (FourthMoment.C:57-76) on float32 [...][4]: float32 [...][14], the four inputs copied,
    then the ten products, each one float32 multiply."""
    s = np.asarray(stokes, np.float32)
    assert s.shape[-1] == 4
    out = np.empty(s.shape[:-1] + (MOM_NDIM,), np.float32)
    out[..., :4] = s
    for k, (i, j) in enumerate(PAIRS):
        out[..., 4 + k] = s[..., i] * s[..., j]             # float32 * float32 -> float32, rounded to nearest
    return out


def geometry(nchan, nbin, runs, ncu=NCU_MI355X):
    """fold_moments_run's launch for a plan: dict of lng (the LONG variant), ngroup (bin groups, grid.x), nseg and seg_samples
    (LONG time segments, grid.z), first / last (the span), and per loader the chunk count and whether the last chunk is ragged."""
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    first, last = plan_span(runs)
    lng = int(runs[:, 2].max()) >= FOLD_LONG_RUN
    ngroup = (nbin + MOM_BPT * MOM_THREADS - 1) // (MOM_BPT * MOM_THREADS)
    if not lng:
        while ngroup < 8 and nchan * ngroup < 512 and nbin // (2 * ngroup) >= 64:
            ngroup *= 2
    nunit = (last - first + MOM_SEG_UNIT - 1) // MOM_SEG_UNIT
    nseg, ups = long_segments(nunit, nchan * ngroup, ncu) if lng else (1, nunit)
    g = dict(lng=lng, ngroup=ngroup, nseg=nseg, seg_samples=ups * MOM_SEG_UNIT, first=first, last=last, max_run=int(runs[:, 2].max()))
    for name, ch in (("stokes", MOM_CHUNK_STOKES), ("stream", MOM_CHUNK_STREAM)):
        g["nchunk_" + name] = (last - first + ch - 1) // ch
        g["ragged_" + name] = (last - first) % ch != 0
    return g


def hand_plan(seed, nbin, n, lo, hi):
    """per-sample bins of runs with random lengths in [lo, hi] (the second of exactly hi) and random bins, each unlike the bin
    before it"""
    rng = np.random.default_rng(seed)
    lens = [int(rng.integers(lo, hi + 1)), hi]
    while sum(lens) < n:
        lens.append(int(rng.integers(lo, hi + 1)))
    lens[-1] -= sum(lens) - n
    assert lens[-1] > 0 and max(lens) == hi
    plan, b = [], -1
    for k in lens:
        nb = int(rng.integers(0, nbin - 1)) if nbin > 1 else 0
        b = nb + (nb >= b) if b >= 0 and nbin > 1 else nb
        plan += [b] * k
    return np.array(plan, np.uint32)


def weighted_runs(plan, idat_start, weights, ndatperweight, weight_idat=0):
    """the runs set_bins_weighted builds (Fold.C:686-716,746-763): sample idat belongs to weight (idat + weight_idat) //
    ndatperweight; a sample of a zero weight is dropped and ends the open run"""
    plan = np.asarray(plan, np.int64)
    idat = idat_start + np.arange(plan.size)
    keep = np.asarray(weights)[(idat + weight_idat) // ndatperweight] != 0
    runs = []
    for i in range(plan.size):
        if not keep[i]:
            continue
        if runs and i > 0 and keep[i - 1] and plan[i - 1] == plan[i]:
            runs[-1][2] += 1
        else:
            runs.append([int(idat[i]), int(plan[i]), 1])
    return np.array(runs, np.int64).reshape(-1, 3), keep


# ---- the exact cases of tests/test_gpu_fourth_moment.py (part c) -------------------------------------------------------------------
# Stokes values are integers in [-8, 8]: a product is at most 64 and a bin takes at most 2^17 samples, so every sum stays below
# 2^23 < 2^24 and is exact in float32 in any order.
# plan: ("bins", phi, samples per bin) through set_bins | ("hand", seed, lo, hi) through set_bin, runs of lo .. hi samples.
# calls: (idat_start, samples) of each fold call into the one profile.  edge: what geometry() must say (test_moments_host.py).
CASES = [
    dict(name="nbin1-long", nchan=2, nbin=1, ndat=3100, plan=("bins", 0.3, 5000.0), calls=[(0, 3100)],
         edge=dict(lng=True, ngroup=1, ragged_stokes=True, ragged_stream=True)),              # one run of 3100 samples
    dict(name="nbin2-runs-of-1", nchan=3, nbin=2, ndat=5002, plan=("bins", 0.1, 1.0), calls=[(1, 5001)],
         edge=dict(lng=False, max_run=1, first_mod4=1, ragged_stokes=True)),
    dict(name="nbin37-start2", nchan=3, nbin=37, ndat=4500, plan=("bins", 0.71, 1.7), calls=[(2, 4490)],
         edge=dict(lng=False, first_mod4=2, nchunk_stokes=3, ragged_stokes=True, ragged_stream=True)),
    dict(name="nbin1024-exact-1chan", nchan=1, nbin=1024, ndat=5000, plan=("bins", 0.52, 0.9), calls=[(0, 5000)],
         edge=dict(lng=False, ngroup=8)),                                                      # one channel: the bins fill the chip
    dict(name="nbin1024-long-segments", nchan=3, nbin=1024, ndat=100000, plan=("bins", 0.05, 70.0), calls=[(4, 99990)],
         edge=dict(lng=True, ngroup=2, nseg_min=8, ragged_stokes=True)),                       # runs of 70 cross segment ends
    dict(name="nbin4097", nchan=2, nbin=4097, ndat=9000, plan=("bins", 0.4, 0.45), calls=[(0, 9000)],
         edge=dict(lng=False, ngroup=9)),                                                      # nine bin groups, the last of one bin
    dict(name="runs-to-63", nchan=3, nbin=64, ndat=6000, plan=("hand", 11, 1, FOLD_LONG_RUN - 1), calls=[(3, 5990)],
         edge=dict(lng=False, max_run=FOLD_LONG_RUN - 1, first_mod4=3)),
    dict(name="runs-to-64", nchan=3, nbin=64, ndat=6000, plan=("hand", 12, 1, FOLD_LONG_RUN), calls=[(5, 5990)],
         edge=dict(lng=True, max_run=FOLD_LONG_RUN, first_mod4=1, nseg_min=2)),
    dict(name="three-calls", nchan=2, nbin=37, ndat=4700, plan=("bins", 0.13, 2.3), calls=[(1, 1500), (1501, 1600), (3101, 1599)],
         edge=dict(lng=False)),
    dict(name="nchan300", nchan=300, nbin=64, ndat=2500, plan=("bins", 0.9, 1.3), calls=[(0, 2500)],
         edge=dict(lng=False, ngroup=1, ragged_stokes=True)),                                  # more channels than compute units
]


def by_name(name):
    (c,) = [c for c in CASES if c["name"] == name]
    return c


def case_stokes(case):
    """the integer Stokes samples of a case, float32 [nchan][1][ndat][4] in [-8, 8]"""
    seed = sum(map(ord, case["name"]))
    return np.random.default_rng(seed).integers(-8, 9, (case["nchan"], 1, case["ndat"], 4)).astype(np.float32)


def case_call_plan(case, k, fold_binplan):
    """(per-sample plan, phi, phase per sample) of fold call k of a case; fold_binplan: the oracle's restatement of the plan
    recurrence.  A "bins" plan starts every call at a phase of its own; a "hand" plan has no phase."""
    idat_start, n = case["calls"][k]
    spec = case["plan"]
    if spec[0] == "hand":
        return hand_plan(spec[1] + k, case["nbin"], n, spec[2], spec[3]), None, None
    phi, pps = spec[1] + 0.37 * k, 1.0 / (spec[2] * case["nbin"])
    return fold_binplan(phi, pps, case["nbin"], n), phi, pps


__all__ = ["CASES", "FOLD_CHUNK", "FOLD_LONG_RUN", "FOLD_MB", "PAIRS", "by_name", "case_call_plan", "case_stokes", "fourth_moment",
           "geometry", "hand_plan", "runs_of_plan", "weighted_runs"]
