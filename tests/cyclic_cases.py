"""The launch arithmetic of cyclic-spectrum folding (dspsr_amd/csrc/cyclic_fold.hip: dspsr_amd_cyclic_fold_set_shape chooses the
number of partial lag arrays, dspsr_amd_cyclic_fold_fold cuts the block into tiles and time segments) restated on the host, and
the cases of tests/test_gpu_cyclic.py built from it.  Kept free of torch so that tests/test_cyclic_cases_host.py can check on a
machine without a GPU that every case reaches the edge it is there for.

A workgroup of k_cyclic_fold is (128 lags, one channel, one time segment) and walks the tiles of its segment with its
accumulators in registers: a run of one bin that crosses a tile boundary stays open, and the run that holds the first step of the
segment comes from a table (tile_first) the host fills.  None of that runs when every segment is one tile long -- which is what
the cases of tests/cyclic_reference.py give -- so the cases here are chosen by partition()."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

import cyclic_reference as cr

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dspsr_amd", "csrc", "cyclic_fold.hip")


def _constants():
    """the constexpr integers of the source, read and not copied: a change there moves partition() with it, and the host test
    then says which case left its edge"""
    text = open(SOURCE).read()
    out = {}
    for name in ("CY_T", "CY_HL", "CY_TARGET_WG", "CY_MAX_PARTS", "CY_PART_BYTES", "CY_MAX_NLAG"):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
        assert m, "%s not found in %s" % (name, SOURCE)
        expr = re.sub(r"(\d)(?:ull|ul|u|ll|l)\b", r"\1", m.group(1).strip(), flags=re.I)
        assert re.fullmatch(r"[\d\s<>*+()-]+", expr), "%s = %s is no integer expression" % (name, m.group(1))
        out[name] = int(eval(expr, {"__builtins__": {}}))
    return out


globals().update(_constants())          # CY_T, CY_HL, CY_TARGET_WG, CY_MAX_PARTS, CY_PART_BYTES, CY_MAX_NLAG
MAX_NCHAN = 65535                        # gridDim.y

Partition = namedtuple("Partition", "nparts ntile nseg tps empty_segments")


def lag_array_bytes(nchan, npol_out, nlag, nbin):
    return nbin * npol_out * nchan * nlag * 2 * 4


def nparts_limits(nchan, npol_out, nlag, nbin):
    """(wanted by the owners, allowed by the bytes): nparts = max(1, min(wanted, CY_MAX_PARTS, allowed))"""
    owners = nchan * -(-nlag // (2 * CY_HL))
    return -(-CY_TARGET_WG // owners), CY_PART_BYTES // lag_array_bytes(nchan, npol_out, nlag, nbin)


def nparts_set_by(nchan, npol_out, nlag, nbin):
    """which term of the clamp gives nparts: "owners", "max" (CY_MAX_PARTS) or "bytes" """
    wanted, allowed = nparts_limits(nchan, npol_out, nlag, nbin)
    if allowed < min(wanted, CY_MAX_PARTS):
        return "bytes"
    return "max" if wanted > CY_MAX_PARTS else "owners"


def partition(nchan, npol_out, nlag, nbin, ndat):
    """(nparts, ntile, nseg, tps, empty_segments) of one fold call on ndat samples; a block of ndat <= nlag launches nothing
    (ntile = nseg = tps = 0).  Segment s walks tiles [s * tps, min((s + 1) * tps, ntile)); the trailing ones may be empty."""
    wanted, allowed = nparts_limits(nchan, npol_out, nlag, nbin)
    nparts = max(1, min(wanted, CY_MAX_PARTS, allowed))
    if ndat <= nlag:
        return Partition(nparts, 0, 0, 0, 0)
    nu = steps(nlag, ndat)
    ntile = -(-nu // CY_T)
    nseg = min(nparts, ntile)
    tps = -(-ntile // nseg)
    return Partition(nparts, ntile, nseg, tps, nseg - -(-ntile // tps))


def steps(nlag, ndat):
    """nu: the steps of skewed time u = idat + ilag / 2 that hold a product"""
    return ndat - nlag + (nlag - 1) // 2


def segment_tiles(p):
    """tiles per segment, in segment order"""
    return [max(0, min((s + 1) * p.tps, p.ntile) - s * p.tps) for s in range(p.nseg)]


# ---- placed plans: the two per-sample plans given directly, changes of bin put on the boundaries of tiles and segments ---------
def plan_of(ndat, changes):
    """per-sample plan from (first sample, bin) pairs in rising order, the first at sample 0"""
    pl = np.zeros(ndat, np.int64)
    assert changes[0][0] == 0 and all(a[0] < b[0] for a, b in zip(changes, changes[1:])) and changes[-1][0] < ndat
    for (u, b), nxt in zip(changes, changes[1:] + [(ndat, 0)]):
        pl[u:nxt[0]] = b
    return pl


def change_points(plan):
    """the samples u at which a run begins (plan[u] != plan[u - 1])"""
    plan = np.asarray(plan)
    return (np.flatnonzero(plan[1:] != plan[:-1]) + 1).tolist()


PLACED_NLAG, PLACED_NBIN, PLACED_NDAT = 33, 8, 4700
PLACED_NU = steps(PLACED_NLAG, PLACED_NDAT)                  # 4683: 10 tiles; with four parts, segments of 3, 3, 3 and 1 tiles
PLACED_SEG1, PLACED_SEG2 = 3 * CY_T, 6 * CY_T                 # first step of segments 1 and 2 when tps = 3
FLIP_FIRST, FLIP_LAST = PLACED_SEG2 + 28, PLACED_SEG2 + 428   # 0, 1, 0, 1, ... inside tile 6


def _edges(bins):
    """The plan with a change of bin at every step the kernel's run walk can get wrong; `bins` renames the eight bins.
      511, 512, 513      runs of one step either side of the first tile boundary: one ends, one begins exactly on it
      1535, 1536, 1537   the same at the first step of segment 1: tile_first[3] must name the run that BEGINS at 1536
      1537 ... 3072      one run over all of segment 1 but its first step: open across two tile boundaries, ends exactly where
                         the segment ends (its sums go to partial array 1 alone)
      3100 ... 3500      bins 0, 1, 0, 1, ...: 400 flushes into the same two bins within tile 6
      3500, 4000         bins 5 and 3 again, seen before in segments 1 and 0: partial arrays 1 and 2, 0 and 2 hold the same bin
      4608               the first step of segment 3
      nu - 1             the last step that holds a product
      nu ... ndat        three more changes: no product is left there, they must change nothing"""
    ch = [(0, 3), (CY_T - 1, 1), (CY_T, 6), (CY_T + 1, 2), (PLACED_SEG1 - 1, 4), (PLACED_SEG1, 7), (PLACED_SEG1 + 1, 5), (PLACED_SEG2, 2)]
    ch += [(u, (u - FLIP_FIRST) % 2) for u in range(FLIP_FIRST, FLIP_LAST)]
    ch += [(FLIP_LAST, 5), (4000, 3), (9 * CY_T, 4), (PLACED_NU - 1, 6), (PLACED_NU, 0), (PLACED_NU + 7, 7), (PLACED_NDAT - 1, 1)]
    return plan_of(PLACED_NDAT, [(u, bins[b]) for u, b in ch])


def placed_plans():
    """(plan0, plan1) of the three calls: the edges on the even lags against one single run on the odd ones, the reverse (bins
    renamed), then both parities at once with different bins"""
    same, mirror = list(range(8)), [7 - b for b in range(8)]
    one = lambda b: np.full(PLACED_NDAT, b, np.int64)
    return [(_edges(same), one(6)), (one(1), _edges(mirror)), (_edges(mirror), _edges(same))]


# ---- the table -----------------------------------------------------------------------------------------------------------------
# One case: a shape and its calls (ndat_fold, idat_start, phi, phase_per_sample, zero_first) as in cyclic_reference.EXACT_CASES,
# with `placed`: per call None (the plan is the phase recurrence) or (plan0, plan1).  1 / (phase_per_sample * nbin) is the length
# of a run in samples.
def _case(name, npol_in, npol_out, nlag, nbin, nchan, calls, placed=None):
    return dict(name=name, npol_in=npol_in, npol_out=npol_out, nlag=nlag, nbin=nbin, nchan=nchan, calls=calls,
                placed=placed or [None] * len(calls))


def _placed_case(name, npol_in, npol_out, nchan):
    pl = placed_plans()
    return _case(name, npol_in, npol_out, PLACED_NLAG, PLACED_NBIN, nchan, [(PLACED_NDAT, 2 * k, 0.0, 0.0, False) for k in range(len(pl))], pl)


CASES = [
    # four parts; call 2: 10 tiles in segments of 3, 3, 3 and 1, runs of 1300 samples stay open across tiles and segments;
    # call 1 (three segments of one tile) leaves sums that call 2 must add to
    _case("multi-tile", 2, 1, 33, 4, 256, [(1100, 0, 0.3, 1.0 / 4 / 700, False), (4700, 2, 0.6, 1.0 / 4 / 1300, False)]),
    # 5 tiles over 4 segments of 2: segment 2 has one tile, segment 3 none (the early return)
    _case("empty-segment", 2, 2, 33, 16, 256, [(2400, 0, 0.2, 1.0 / 16 / 9.3, False)]),
    # 400 owners: three parts; lags 128 and 129 are one active lane in each wave of the second workgroup
    _case("three-parts", 1, 1, 130, 8, 200, [(3300, 4, 0.45, 1.0 / 8 / 40, False)]),
    # 1024 owners: ONE part, lagdata == parts, no combine; four tiles in the one segment; 2.3 bins per sample: every run is one
    # step long and the two parities follow different lists
    _case("one-part", 1, 1, 3, 7, 1024, [(1700, 0, 0.2, 2.3 / 7, False), (600, 0, 0.7, 1.0 / 7 / 50, False)]),
    # both waves full (128), two full workgroups (256).  64 parts > 4 tiles: tps is 1 here by construction -- these two are
    # about the lanes, not about the tiles
    _case("nlag128", 2, 4, 128, 32, 5, [(1800, 0, 0.1, 1.0 / 32 / 11, False)]),
    _case("nlag256", 2, 4, 256, 32, 5, [(1800, 0, 0.1, 1.0 / 32 / 11, False)]),
    # the largest nlag: grid.x 512, h0 up to 32704, two parts of 34 and 33 tiles; most X windows are all zero
    _case("max-nlag", 1, 1, CY_MAX_NLAG, 8, 1, [(CY_MAX_NLAG + 1100, 0, 0.3, 1.0 / 8 / 300, False)]),
    # the largest nchan: grid.y 65535, one part, two tiles in the one segment
    _case("max-nchan", 1, 1, 2, 2, MAX_NCHAN, [(530, 0, 0.4, 1.0 / 2 / 100, False)]),
    # one lag array of 67.6 MB: the 2 GiB of CY_PART_BYTES allow 31 parts, not 64; 41 tiles in segments of 2: 21 used, 10 empty
    _case("part-cap", 2, 4, 129, 16384, 1, [(129 + 512 * 40, 0, 0.9, 1.0 / 16384 / 3.1, False)]),
    # the placed plans where four segments walk 3, 3, 3 and 1 tiles, and once more with one part (one segment of 10 tiles: the
    # tile_first table is read at tile 0 alone, every other boundary is the kernel's own walk)
    _placed_case("placed-four-parts", 2, 2, 256),
    _placed_case("placed-one-part", 1, 1, 1024),
]
NAMES = [c["name"] for c in CASES]


def by_name(name):
    return CASES[NAMES.index(name)]


def call_plans(case, k):
    """(plan0, plan1, hits) of call k: the placed plans, or the phase recurrence"""
    ndat, _start, phi, pps, _zero = case["calls"][k]
    if case["placed"][k] is None:
        return cr.plans(phi, pps, case["nbin"], ndat)
    p0, p1 = case["placed"][k]
    return p0, p1, np.bincount(p0, minlength=case["nbin"]).astype(np.uint32)


def case_rows(name, k):
    """the input of call k: exact integer data, idat_start samples in front of the block"""
    case = by_name(name)
    ndat, start = case["calls"][k][:2]
    return cr.exact_rows(7000 + 10 * NAMES.index(name) + k, case["nchan"], case["npol_in"], start + ndat)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float32):
    """[(hits, lag array after the call)] per call of the case, in `dtype` arithmetic; computed once per process"""
    case = by_name(name)
    cr.check_exact(case)
    lags, steps_ = None, []
    for k, (ndat, start, _phi, _pps, zero) in enumerate(case["calls"]):
        p0, p1, hits = call_plans(case, k)
        if zero:
            lags = None
        lags = cr.fold(case_rows(name, k)[:, :, start:], p0, p1, case["nlag"], case["npol_out"], case["nbin"], lags, dtype)
        steps_.append((hits, lags))
    return steps_
