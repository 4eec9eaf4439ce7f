"""The fold inside the last filterbank pass (dspsr_amd_filterbank_perform_fold: k_inv_chan<., FOLD> of csrc/fb_inv_chan.h, its
two-pass twin k_rows_inv<., ., FOLD> of csrc/fb_two_pass.hip, their item walk csrc/fb_inv_walk.h and fold csrc/fb_inv_epilogue.h, fb_launch_fused of csrc/filterbank.hip, the part plan of csrc/fold_plan.h
and fold_combine_partials of csrc/fold.hip): the host's geometry and launch arithmetic restated, and the cases of
tests/test_gpu_fused_fold.py as plain data with a computed record of the branches each one reaches.  No torch: the host test
tests/test_fused_fold_cases_host.py checks on a machine without a GPU that every case reaches what its name says.

A case is one filterbank object, one fold profile and a list of calls; every call has its parts and its plan, given as runs
(first sample, bin, samples) in time order -- from the phase recurrence of Fold.C:744-787 (`phase`) or made by hand (`hand`, fed
through set_bin sample by sample; a gap in a hand-made plan is a stretch of zero weight)."""
import functools
import math
import os
import re

import numpy as np

from fold_reference import FOLD_LONG_RUN, fused_fold_model, fused_nseg, fused_runs_of_launch, runs_of_plan

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dspsr_amd", "csrc")
FUSED_AUTO, FUSED_ALWAYS, FUSED_NEVER = 0, 1, 2          # dspsr_amd/_lib.py


def _constant(header, name):
    """a constexpr integer of the sources, read and not copied: a change there moves the records with it"""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, "%s not found in %s" % (name, header)
    return int(m.group(1))


FB_PSL_MAX = _constant("fb_common.h", "FB_PSL_MAX")                  # part offsets a workgroup keeps in LDS
FOLD_FUSED_MAX_RUN = _constant("fold_internal.h", "FOLD_FUSED_MAX_RUN")
LOG_POINTS = _constant("filterbank.hip", "LOG_POINTS_DEFAULT")
MAX_LOGF = _constant("fb_common.h", "MAX_LOGF")
PTS = _constant("wgfft.h", "PTS")
LDS_BYTES = 160 * 1024


# ---- geometry (filterbank.hip fb_init_geom, fb_tile, fb_pick_kernels, fb_setup_two_pass; wgfft.h) --------------------------------
def _ltw_entries(logf):
    nq, rem = divmod(logf, 4)
    return sum(4 << (logf - 4 * (st + 1)) for st in range(nq - (0 if rem else 1)))


def _lds_bytes(points, logf):
    return (points + ((points >> 6) << 2) + 8 + _ltw_entries(logf) + 8 + 16) * 8


def plan_lds_cap(lds, clamp):
    """fb_common.h fb_plan_lds: plan entries per LDS buffer behind the plain kernel's `lds` bytes"""
    psl = FB_PSL_MAX * 4
    cap = (LDS_BYTES - 64 - lds - 16 - psl) // 32 if lds + 64 + 16 + psl < LDS_BYTES else 0
    cap = min(cap, clamp)
    return cap if cap >= 16 else 0


def _stages(logf):
    return logf // 4 + (1 if logf % 4 else 0)        # wgfft.h FftPlan::NS


def geometry(C, M, nfilt, real, force_four_pass=0, raw8=True):
    """What dspsr_amd_filterbank_create builds for nchan_subband C (2^k or 3 * 2^k), freq_res M (2^k), dual polarisation; raw8:
    the calls bring the generic 8-bit block (the two-pass path is taken per call, fb_takes_two_pass)."""
    nsub = 3 if C % 3 == 0 else 1
    L = (2 if real else 1) * C * M
    logM, logR, logC = int(math.log2(M)), int(math.log2(L // nsub // M)), int(math.log2(C // nsub))
    assert 1 << logM == M and (1 << logR) * nsub * M == L
    g = dict(C=C, M=M, nkeep=M - sum(nfilt), real=real, nsub=nsub, logM=logM)
    three = logM <= MAX_LOGF and logR <= MAX_LOGF and force_four_pass != 1
    if three:
        logT1, logT2 = min(logR, LOG_POINTS - logM), min(logM, LOG_POINTS - logR)
        logX3 = min(logC, max(0, LOG_POINTS - logM - 1))
        logT3 = logX3                                                      # fb_tile: "pass-3 tile = one layout block"
        p1, p2, p3 = M << logT1, (1 << logR) << logT2, (M << logT3) << 1
        three = not (p1 < 32 or p2 < 32 or p3 < 32 or p3 > 1 << LOG_POINTS or logT1 < 1 or logT2 < 1)
    if not three:
        # four passes: lma_best is restated for the sizes the cases use only; elsewhere the record stops at `passes`
        g.update(passes=4, tiles=None, plan_cap=0)
        lma = {14: 6, 15: 7, 16: 8, 17: 9, 18: 10}.get(logM)
        if nsub == 1 and lma is not None:
            g["logTt"] = min(lma, LOG_POINTS - 1 - (logM - lma))
        return g
    nt3 = p3 // PTS
    lds3 = _lds_bytes(p3, logM)
    # fb_pick_kernels / fb_common.h full_logt: the full-size tile takes k_inv_chan<., ., LOGT = 14 - logM>, whose tile is
    # LOGT - 1 and not g.logT3; it is picked only where logT3 + 1 == LOGT, so the kernel's logT3 is the host's either way
    full_logt = 14 - logM if 14 - logM >= 1 else -1
    g["kernel_logT3"] = full_logt - 1 if logT3 + 1 == full_logt else logT3
    g.update(passes=3, logT3=logT3, logX3=logX3, T3=1 << logT3, tiles=C >> logT3, blockdim=nt3, lds3=lds3,
             wg3=2 if 2 * lds3 + 1024 <= LDS_BYTES else 1, plan_cap=plan_lds_cap(lds3, nt3), stages=_stages(logM))
    lfb = 13 - logM
    lfa = int(math.log2(L)) - lfb
    if nsub == 1 and not real and force_four_pass != 2 and 9 <= logM <= 12 and logM <= lfa <= 14 and raw8:
        # k_rows_inv: tiles of Fb = 2^13 / M channels, 512 threads, one workgroup per compute unit
        g.update(passes=2, T3=1 << lfb, tiles=C >> lfb, blockdim=512, wg3=1, plan_cap=plan_lds_cap(_lds_bytes(1 << 14, logM), 512))
    return g


def grid_for(items, ncu):
    """filterbank.hip grid_for: persistent grids, a multiple of 8 from 8 workgroups on"""
    gsz = min(items, ncu)
    return gsz & ~7 if gsz >= 8 else gsz


def fold_b_permutation(grid, lr):
    """fb_inv_walk.h (xcd_lr): the tile of workgroup b in an exact launch (nseg == 1): blocks b, b + 8, ... of one X layout block of
    2^lr tiles; the identity unless lr > 0 and the grid is a multiple of 8 << lr"""
    b = np.arange(grid, dtype=np.int64)
    if lr > 0 and grid & ((8 << lr) - 1) == 0:
        return ((((b >> (3 + lr)) << 3) | (b & 7)) << lr) | ((b >> 3) & ((1 << lr) - 1))
    return b


def fold_mode(g, policy, ncu):
    """dspsr_amd_filterbank_fold_is_fused"""
    if g["passes"] == 4:
        return 3 if policy != FUSED_NEVER and g["logTt"] >= 3 and (2 * g["nkeep"] >= g["M"] or policy == FUSED_ALWAYS) else 0
    if g["nkeep"] >= 65536:
        return 0
    if policy != FUSED_AUTO:
        return 1 if policy == FUSED_ALWAYS else 0
    tiles = g["C"] >> g["logT3"]                  # (the three-pass tile count, also for calls that take two passes)
    return 1 if tiles >= ncu else 2 if tiles >= 8 else 0


# ---- plans -----------------------------------------------------------------------------------------------------------------------
def phase_plan(phi, pps, nbin, ndat):
    """per-sample bins of the double recurrence of Fold.C:744-787"""
    plan = np.empty(ndat, np.int64)
    fn = float(nbin)
    for i in range(ndat):
        phi -= math.floor(phi)
        plan[i] = int(phi * fn)
        phi += pps
    assert plan.max() < nbin
    return plan


def runs_of(plan, nbin):
    """runs (first sample, bin, samples) of a per-sample plan; nbin marks a dropped sample: a dropped sample ends the open run"""
    r = runs_of_plan(plan)
    return r[r[:, 1] < nbin]


def hand_runs(pieces):
    """runs from (bin, samples) pieces laid one after the other; bin None leaves a gap of that many samples"""
    out, t = [], 0
    for b, n in pieces:
        if b is not None:
            out.append((t, b, n))
        t += n
    r = np.array(out, np.int64).reshape(-1, 3)
    # set_bin opens a run where the bin CHANGES: two runs of one bin in a row (with or without a gap) would be read as one
    assert (r[1:, 1] != r[:-1, 1]).all(), "neighbouring runs of a hand-made plan need different bins"
    return r, t


def part_plan(runs, nkeep, npart, nbin):
    """fold_plan.h part_plan_count / part_plan_fill restated (tests/test_fold_plan_host.py compares the two): per part the
    list of active bins, each with its intervals (offset in the part, hits) in time order -- runs cut at every multiple of nkeep, bucketed by (part, bin)"""
    parts = [dict() for _ in range(npart)]
    for off, b, n in np.asarray(runs, np.int64).reshape(-1, 3):
        off, left = int(off), int(n)
        while left:
            p, within = divmod(off, nkeep)
            m = min(left, nkeep - within)
            assert p < npart, "plan sample beyond the parts of the call"
            parts[p].setdefault(int(b), []).append((within, m))
            off += m
            left -= m
    return [sorted(d.items()) for d in parts]


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _case(name, group, C, M, nfilt, real, calls, nbin, max_parts, policy, prof="4", input_nchan=1, four=0, bound=None):
    """calls: [(parts, plan)] with plan ("phase", phi, pps) | ("hand", pieces);
    prof: "4" (npol 1 x ndim 4) or "2x2"; bound: None (the library's profile) or (offset floats, row padding floats) of a
    caller's buffer filled with NaN around the rows; four: force_four_pass"""
    return dict(name=name, group=group, C=C, M=M, nfilt=nfilt, real=real, calls=calls, nbin=nbin, max_parts=max_parts, policy=policy,
                prof=prof, input_nchan=input_nchan, four=four, bound=bound)


PSL = dict(C=32, M=256, nfilt=(100, 92), real=True)              # ONE tile of 32 channels, nkeep 64
PSL2 = dict(C=64, M=256, nfilt=(100, 92), real=True)             # two tiles
PSL2P = dict(C=16, M=512, nfilt=(40, 3), real=False)            # two passes (8-bit complex), ONE tile of 16 channels, nkeep 469
SEG3 = dict(C=64, M=1024, nfilt=(500, 484), real=True)           # three passes, 8 tiles of 8 channels, nkeep 40
SEG2 = dict(C=32, M=2048, nfilt=(1000, 1000), real=False)        # two passes (8-bit complex), 8 tiles of 4 channels, nkeep 48
SEG16 = dict(C=32, M=4096, nfilt=(2040, 2016), real=True)        # three passes, 16 tiles of 2 channels, nkeep 40
CAP = dict(C=2, M=8192, nfilt=(96, 96), real=True)               # two tiles of ONE channel, nkeep 8000, 512 threads
RUNS = dict(C=16, M=1024, nfilt=(100, 124), real=True)           # two tiles of 8 channels, nkeep 800
FOUR = dict(C=4, M=16384, nfilt=(301, 212), real=True)           # four passes, segments of 32 samples


def _ph(parts, nkeep, nbin, per_bin, phi0, k=0):
    """call k of a stream folded with `per_bin` samples per bin: the phase continues from call to call"""
    pps = 1.0 / (nbin * per_bin)
    return (parts, ("phase", (phi0 + k * pps * nkeep * 37) % 1.0, pps))


def _cap_pieces(cap, blockdim, nkeep):
    """six parts whose active bins number cap - 1, cap, cap + 1, blockdim + 1 (one work item more than threads: T3 = 1), 3 and
    cap again; runs of 3 samples round the part's bins, so every bin has several intervals"""
    pieces = []
    for k, nact in enumerate((cap - 1, cap, cap + 1, blockdim + 1, 3, cap)):
        bins = [(11 * k + 7 * i) % 600 for i in range(nact)]          # 7 and 600 coprime: nact distinct bins
        t = 0
        i = 0
        while t < nkeep:
            n = min(3, nkeep - t)
            pieces.append((bins[i % nact], n))
            t += n
            i += 1
    return pieces


def _runs_pieces(nkeep):
    """five parts.  Part 0: first intervals of 1, 7, 8, 9, 16 and 17 hits (the 8-at-a-time loop and its tail), bins 0-5, then
    bins 0 and 1 again (nint 2) and bin 0 once more (nint 3), the rest in bins 6 and 7 in turn; part 1: bins 11 and 12 in turn; part 2: EMPTY (a
    zero-weight stretch of exactly one part in the middle of the launch); part 3: bin 0 again; part 4: short runs"""
    p0 = [(0, 1), (1, 7), (2, 8), (3, 9), (4, 16), (5, 17), (0, 5), (1, 24), (0, 33)]
    rest = nkeep - sum(n for _, n in p0)
    p0 += [(6 + i % 2, 20) for i in range(rest // 20)]
    assert rest % 20 == 0 and nkeep % 50 == 0 and nkeep % 10 == 0
    p1 = [(11 + i % 2, 50) for i in range(nkeep // 50)]
    p3 = [(0, 100)] + [(9 + i % 2, 50) for i in range((nkeep - 100) // 50)]
    p4 = [(i % 5, 10) for i in range(nkeep // 10)]
    return p0 + p1 + [(None, nkeep)] + p3 + p4


def _long_pieces(nkeep, longest):
    """two parts: a run of `longest` samples inside part 0, short runs around it"""
    rest = 2 * nkeep - longest - 40
    tail = [(8, rest % 20)] if rest % 20 else []
    return [(1, 40), (2, longest)] + [(3 + i % 4, 20) for i in range(rest // 20)] + tail


def _seg_empty_pieces(nkeep):
    """24 parts (16 runs of 2, runs 12-15 empty): part 2 -- the FIRST part of run 1 -- and part 7 hold no sample"""
    pieces = []
    for p in range(24):
        if p in (2, 7):
            pieces.append((None, nkeep))
        else:
            pieces += [((3 * p + i) % 16, 8) for i in range(nkeep // 8)]
    return pieces


def _cases():
    A, N = FUSED_ALWAYS, FUSED_NEVER
    out = []
    # -- psl: ONE exact launch of 127, 128, 130 parts: fnp + 1 = 128 (offsets in LDS), 129 and 131 (global memory, no DMA, no PRE)
    for n, geo in ((127, PSL), (128, PSL), (130, PSL2)):
        for prof in ("4", "2x2"):
            out.append(_case("psl-%d-%s" % (n, prof), "psl", calls=[_ph(n, 64, 64, 1.7, 0.13)], nbin=64, max_parts=130, policy=A, prof=prof, **geo))
    # two launches of 129 parts in one call: the second one has part0 = 129 and its offsets in global memory
    out.append(_case("psl-2x129-4", "psl", calls=[_ph(258, 64, 64, 1.7, 0.13)], nbin=64, max_parts=129, policy=A, **PSL))
    # the two-pass twin (k_rows_inv): some 276 bins x 16 channels on 512 threads, nine items per thread
    out.append(_case("psl-127-2pass", "psl", calls=[_ph(127, 469, 512, 1.7, 0.13)], nbin=512, max_parts=130, policy=A, **PSL2P))
    out.append(_case("psl-128-2pass", "psl", calls=[_ph(128, 469, 512, 1.7, 0.13)], nbin=512, max_parts=130, policy=A, prof="2x2", **PSL2P))
    out.append(_case("psl-2x129-2pass", "psl", calls=[_ph(258, 469, 512, 1.7, 0.13)], nbin=512, max_parts=129, policy=A, **PSL2P))
    # -- seg-ragged: mode 2, two or three calls into one profile, launches of 1, 2, 11, 16, 17, 24 and 37 parts
    seg = [("3pass-real-a", SEG3, [37, 24], 37, "4", 1, 0), ("3pass-real-b", SEG3, [17, 11, 2], 37, "2x2", 1, 0),
           ("3pass-real-c", SEG3, [16, 1, 37], 16, "4", 1, 0),                     # 37 parts in launches of 16, 16 and 5
           ("3pass-16tiles", SEG16, [37, 17], 37, "2x2", 1, 0),
           ("2pass-a", SEG2, [37, 17], 37, "4", 1, 0), ("2pass-b", SEG2, [24, 2, 1], 37, "2x2", 1, 0),
           ("3pass-complex", SEG2, [11, 37], 37, "4", 1, 2),                       # force_four_pass = 2: never the two-pass path
           ("2pass-nchan3", SEG2, [24, 17], 37, "2x2", 3, 0), ("3pass-complex-nchan3", SEG2, [16, 37], 37, "4", 3, 2)]
    for name, geo, parts, mp, prof, inch, four in seg:
        nk = geo["M"] - sum(geo["nfilt"])
        out.append(_case("seg-" + name, "seg", calls=[_ph(n, nk, 32, 1.3, 0.21, k) for k, n in enumerate(parts)], nbin=32, max_parts=mp,
                         policy=FUSED_AUTO, prof=prof, input_nchan=inch, four=four, **geo))
    out.append(_case("seg-empty-part", "seg", calls=[_ph(11, 40, 16, 2.1, 0.4), (24, ("hand", _seg_empty_pieces(40)))], nbin=16, max_parts=37,
                     policy=FUSED_AUTO, **SEG3))
    # -- cap: active bins of a part either side of plan_cap, and one work item more than the workgroup has threads
    g = geometry(**CAP)
    out.append(_case("cap-around", "cap", calls=[(6, ("hand", _cap_pieces(g["plan_cap"], g["blockdim"], g["nkeep"])))], nbin=600, max_parts=8,
                     policy=A, **CAP))
    out.append(_case("cap-around-2x2", "cap", calls=[(6, ("hand", _cap_pieces(g["plan_cap"], g["blockdim"], g["nkeep"])))], nbin=600, max_parts=3,
                     policy=A, prof="2x2", **CAP))
    # -- runs
    out.append(_case("runs-hits", "runs", calls=[(5, ("hand", _runs_pieces(800))), _ph(3, 800, 40, 9.0, 0.7)], nbin=40, max_parts=8, policy=A, **RUNS))
    out.append(_case("runs-hits-2x2", "runs", calls=[(5, ("hand", _runs_pieces(800)))], nbin=40, max_parts=2, policy=A, prof="2x2", **RUNS))
    out.append(_case("runs-639", "runs", calls=[_ph(2, 800, 16, 3.0, 0.1), (2, ("hand", _long_pieces(800, FOLD_FUSED_MAX_RUN - 1)))], nbin=16,
                     max_parts=2, policy=A, **RUNS))
    out.append(_case("runs-640", "runs", calls=[_ph(2, 800, 16, 3.0, 0.1), (2, ("hand", _long_pieces(800, FOLD_FUSED_MAX_RUN)))], nbin=16,
                     max_parts=2, policy=A, **RUNS))
    # -- placement: bound profiles, (offset, row padding) in floats; rows of nbin * ndim floats
    for name, prof, bound in (("4-span4", "4", (0, 4)), ("4-even", "4", (0, 2)), ("4-odd", "4", (0, 3)), ("4-off1", "4", (1, 4)),
                              ("2x2-span4", "2x2", (0, 0)), ("2x2-even", "2x2", (0, 2)), ("2x2-odd", "2x2", (0, 1)), ("2x2-off1", "2x2", (1, 2))):
        out.append(_case("place-" + name, "placement", calls=[_ph(5, 64, 50, 1.7, 0.3, k) for k in range(2)], nbin=50, max_parts=2, policy=A,
                         prof=prof, bound=bound, **PSL))
    # -- grids: an exact launch where some workgroups walk two tiles (12 tiles on a grid of 8: not a multiple of 8), and its
    #    neighbour of 16 tiles on a grid of 16
    out.append(_case("grid-12-tiles", "grid", C=96, M=1024, nfilt=(500, 484), real=True, calls=[_ph(3, 40, 32, 1.3, 0.6), _ph(2, 40, 32, 1.3, 0.6, 1)],
                     nbin=32, max_parts=2, policy=A))
    out.append(_case("grid-16-tiles", "grid", calls=[_ph(3, 40, 32, 1.3, 0.6), _ph(2, 40, 32, 1.3, 0.6, 1)], nbin=32, max_parts=2, policy=A,
                     prof="2x2", **SEG16))
    # -- segment sums (fold_is_fused() == 3): the three-way qualification of the four-pass plan, segments of 32 samples
    nk = FOUR["M"] - sum(FOUR["nfilt"])
    for name, odd, short in (("exact", 32, 0), ("one-short-interval", 31, 0), ("one-sample-short", 32, 1)):
        out.append(_case("segsum-" + name, "segsum", calls=[(5, ("hand", _segsum_pieces(5 * nk, 32, odd, short)))], nbin=64, max_parts=2,
                         policy=FUSED_AUTO, **FOUR))
    return out


def _segsum_pieces(ndat, seg, odd, short):
    """a first run of 100 samples (long enough for the segment-sum path), inner runs of exactly `seg` samples -- the tenth of
    `odd` --, the last run up to the end of the call less `short` samples"""
    pieces, t, i = [(0, 100)], 100, 1
    while ndat - short - t > 2 * seg:
        n = odd if i == 10 else seg
        pieces.append((i % 64, n))
        t += n
        i += 1
    pieces.append((i % 64, ndat - short - t))
    if short:
        pieces.append((None, short))
    return pieces


CASES = _cases()
NAMES = [c["name"] for c in CASES]


def by_name(name):
    return CASES[NAMES.index(name)]


def of_group(group):
    return [c["name"] for c in CASES if c["group"] == group]


@functools.lru_cache(maxsize=None)
def call_runs(name, k):
    """(runs, per-bin hits, samples) of call k"""
    c = by_name(name)
    parts, plan = c["calls"][k]
    ndat = parts * (c["M"] - sum(c["nfilt"]))
    if plan[0] == "hand":
        runs, t = hand_runs(plan[1])
        assert t == ndat, (name, k, t, ndat)
    else:
        runs = runs_of(phase_plan(plan[1], plan[2], c["nbin"], ndat), c["nbin"])
    hits = np.zeros(c["nbin"], np.int64)
    np.add.at(hits, runs[:, 1], runs[:, 2])
    return runs, hits.astype(np.uint32), ndat


def launches_of(parts, max_parts):
    """fb_group_parts for these small shapes: min(left, max_parts)"""
    out = []
    while parts:
        out.append(min(parts, max_parts))
        parts -= out[-1]
    return out


def dispatch(c, g, k, ncu):
    """which path dspsr_amd_filterbank_perform_fold takes for call k: "fused" (mode 1 or 2), "segsum" (mode 3, the plan
    qualifies) or "detect+fold"; with the stand-alone fold's association ("time" | "long")"""
    runs, _hits, ndat = call_runs(c["name"], k)
    mode = fold_mode(g, c["policy"], ncu)
    planes2 = c["prof"] == "2x2"
    off, pad = c["bound"] or (0, 0)
    span = c["nbin"] * (2 if planes2 else 4) + pad
    vec4 = off % 4 == 0 and span % (2 if planes2 else 4) == 0          # (the buffers of the tests start on a 256-byte boundary)
    max_run = int(runs[:, 2].max()) if len(runs) else 0
    if mode == 3 and not planes2 and vec4 and max_run >= FOLD_LONG_RUN:
        seg = 1 << g["logTt"]
        cover = len(runs) and runs[0, 0] == 0 and (runs[1:, 0] == runs[:-1, 0] + runs[:-1, 2]).all() and runs[-1, 0] + runs[-1, 2] == ndat
        if cover and (runs[1:-1, 2] >= seg).all():
            return "segsum", None
    if mode in (1, 2) and vec4 and max_run < FOLD_FUSED_MAX_RUN:
        return "fused", None
    # (the stand-alone fold reads the library's own detected block: aligned rows, so runs of FOLD_LONG_RUN samples take the
    #  long-run kernel whatever the profile's placement)
    return "detect+fold", "long" if max_run >= FOLD_LONG_RUN else "time"


@functools.lru_cache(maxsize=None)
def record(name, ncu=256, wg3=None):
    """What the case reaches, worked out from the restated host code for a device of `ncu` compute units (wg3: override the
    workgroups per compute unit, to show that a record does not depend on it)."""
    c = by_name(name)
    g = geometry(c["C"], c["M"], c["nfilt"], c["real"], c["four"])
    mode = fold_mode(g, c["policy"], ncu)
    rec = dict(mode=mode, passes=g["passes"], tiles=g["tiles"], plan_cap=g["plan_cap"], blockdim=g.get("blockdim"), T3=g.get("T3"), calls=[])
    if g["passes"] == 4:
        rec["seg"] = 1 << g["logTt"]
        for k in range(len(c["calls"])):
            runs = call_runs(name, k)[0]
            rec["calls"].append(dict(path=dispatch(c, g, k, ncu)[0], max_run=int(runs[:, 2].max()), inner=sorted(set(runs[1:-1, 2].tolist())),
                                     end=int(runs[-1, 0] + runs[-1, 2])))
        return rec
    wgs = ncu * (g["wg3"] if wg3 is None else wg3) if g["passes"] == 3 else ncu
    rec["wgs"] = wgs
    rec["grid_exact"] = grid_for(g["tiles"], wgs)
    rec["lr"] = g["logX3"] - g["kernel_logT3"]                 # fb_inv_chan.h (the xcd_lr it hands to inv_walk): lr = logX3 - logT3 with the KERNEL's logT3
    for k, (parts, _plan) in enumerate(c["calls"]):
        runs, _hits, _ndat = call_runs(name, k)
        path, assoc = dispatch(c, g, k, ncu)
        call = dict(path=path, assoc=assoc, launches=[], max_run=int(runs[:, 2].max()))
        if path == "fused":
            pp = part_plan(runs, g["nkeep"], parts, c["nbin"])
            part0 = 0
            for ns in launches_of(parts, c["max_parts"]):
                nseg = fused_nseg(ns, g["tiles"], wgs) if mode == 2 else 1
                rr = fused_runs_of_launch(ns, nseg)
                nact = [len(pp[part0 + p]) for p in range(ns)]
                # per part: the offsets of its run sit in LDS (fb_inv_epilogue.h InvPlan::use_psl); then, and only then, its entries can (dma_ok)
                part_psl = [g["plan_cap"] > 0 and n + 1 <= FB_PSL_MAX for _p0, n in rr for _ in range(n)]
                in_lds = [g["stages"] >= 2 and u and a <= g["plan_cap"] for u, a in zip(part_psl, nact)]
                items = [-(-(a * g["T3"]) // g["blockdim"]) for a in nact]
                first_hits = sorted({iv[0][1] for p in range(ns) for _b, iv in pp[part0 + p]})
                call["launches"].append(dict(
                    ns=ns, nseg=nseg, fpps=-(-ns // nseg), run_parts=[n for _p0, n in rr], empty_runs=[s for s, (_p0, n) in enumerate(rr) if n == 0],
                    psl=[n + 1 for _p0, n in rr if n], use_psl=[g["plan_cap"] > 0 and n + 1 <= FB_PSL_MAX for _p0, n in rr if n],
                    nact=nact, in_lds=in_lds, items_per_thread=items,
                    # `pre` of the kernels is in_lds: a part where a thread holds a prefetched accumulator AND has a second item
                    second_item_with_pre=[p for p in range(ns) if in_lds[p] and items[p] >= 2],
                    nint=sorted({len(iv) for p in range(ns) for _b, iv in pp[part0 + p]}), first_hits=first_hits,
                    empty_parts=[p for p in range(ns) if nact[p] == 0], run_first_parts=[p0 for p0, n in rr if n],
                    grid=g["tiles"] * nseg if nseg > 1 else grid_for(g["tiles"], wgs)))
                part0 += ns
        rec["calls"].append(call)
    return rec


def model_of_call(cfg, det, runs, profile, parts, ncu):
    """(fold_is_fused(), fused_fold_model) of ONE perform_fold of `parts` parts of the 8-bit block into the library's own profile,
    by an object created with `cfg` (the fields of dspsr_amd_filterbank_config) on a device of `ncu` compute units; the model is
    None where the call does not take the fused kernels (mode 0 or 3, or a run of FOLD_FUSED_MAX_RUN samples)"""
    g = geometry(cfg.nchan_subband, cfg.freq_res, (cfg.nfilt_pos, cfg.nfilt_neg), bool(cfg.real_input), cfg.force_four_pass)
    mode = fold_mode(g, cfg.fused_fold, ncu)
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    if mode not in (1, 2) or (len(runs) and int(runs[:, 2].max()) >= FOLD_FUSED_MAX_RUN):
        return mode, None
    wgs = ncu * g["wg3"] if g["passes"] == 3 else ncu
    return mode, fused_fold_model(det, runs, profile, g["nkeep"], launches_of(parts, cfg.max_parts), mode,
                                  lambda ns: fused_nseg(ns, g["tiles"], wgs))


def loadtofold_block_model(lt, raw, npart, profile, ncu):
    """(mode, hits, model) of the block pipeline.LoadToFold `lt` is about to fold with process_block(raw, npart), its fold being
    one fused call over the whole block: the plan as LoadToFold._plan_piece makes it, the detected samples from perform_detect of
    the pipeline's own filterbank object on the same block.  Call it BEFORE process_block.  The phase of the first sample is
    the pipeline's own (lt._phase, out_start, ndat_out): this checks the ORDER of the sums, not the phase law -- that stays with
    the callers' hits comparison against Detection + Fold.  (The one place of this module that
    needs torch and a device; imported here so that the table stays importable without either.)"""
    import torch
    import dspsr_amd
    ndat, nbin = npart * lt.nkeep, lt.cfg.nbin
    phi, pfold = lt._phase(lt.out_start + (lt.ndat_out + 0.5) / lt.out_rate)
    plan, hits = dspsr_amd.fold_binplan(phi, (1.0 / lt.out_rate) / pfold, nbin, ndat)
    det = torch.zeros((lt.nchan_out, 1, 4 * ndat), dtype=torch.float32, device=raw.device)
    lt.fb.perform_detect(det, npart, dspsr_amd.COHERENCE, 4, raw=raw, layout=lt.layout, scale=lt.scale8)
    mode, model = model_of_call(lt.fb.cfg, det.view(lt.nchan_out, ndat, 4).cpu().numpy(), runs_of_plan(plan.astype(np.int64)), profile, npart, ncu)
    return mode, hits, model


def raw_bytes(c, parts):
    """bytes of the 8-bit block of a call of `parts` parts: parts * step + overlap samples of two polarisations of every input
    channel, one byte per real sample, two per complex one"""
    nfilt = sum(c["nfilt"])
    samples = (2 if c["real"] else 1) * c["C"] * (parts * (c["M"] - nfilt) + nfilt)
    return samples * c["input_nchan"] * 2 * (1 if c["real"] else 2)
