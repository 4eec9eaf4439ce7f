"""CPU restatement of the stand-alone fold (dspsr_amd_fold_fold, csrc/fold.hip) for the tests: the sums of every kernel in the
association that kernel uses, in float32, and the host's choice of kernel.

A plan is its list of runs (first sample, phase bin, samples) in time order, as set_bin / set_bins build it; `rows` are the
detected samples [nchan][npol][ndat][ndim] (sample idat of a row at rows[:, :, idat, :]); `prof` the profile
[nchan][npol][nbin][ndim] before the fold.  The functions return the profile after it and leave `prof` as it was.

- fold_time_order: the CPU loop of Fold.C:844-852, every (chan, pol, bin, dim) sum in strict time order.  The association of
  k_fold_direct, k_fold_chunked<., false, .> and k_fold_dense.
- fold_long_model: the association of k_fold_chunked<., true, .> + k_fold_combine (the LONG path), bit for bit.
- fold_dispatch: which kernel dspsr_amd_fold_fold launches for a call, with its template arguments and launch shape (fold_plan.h
  fold_shape); fold_many_dispatch: the shape of a shared launch (fold_many_shape).
- fused_fold_model: the fold inside the last filterbank pass (dspsr_amd_filterbank_perform_fold, fold_is_fused() 1 and 2).
"""
import numpy as np

FOLD_CHUNK = 2048        # samples per chunk (fold_plan.h FOLD_CHUNK)
FOLD_MB = 32             # samples per micro-block (fold_plan.h FOLD_MB)
FOLD_BPT = 4             # bins per thread (fold_plan.h FOLD_BPT)
FOLD_MANY_THREADS = 512  # threads of a k_fold_many workgroup at most (fold_plan.h FOLD_MANY_THREADS)
FOLD_LONG_RUN = 64       # a run this long selects the LONG path (fold_plan.h FOLD_LONG_RUN)


def runs_of_plan(plan, idat_start=0):
    """The runs set_bin builds from a per-sample bin plan (a new run wherever the bin changes): int64 [nrun][3] of
    (first sample, bin, samples), samples counted from idat_start."""
    plan = np.asarray(plan)
    if plan.size == 0:
        return np.zeros((0, 3), np.int64)
    starts = np.concatenate(([0], np.flatnonzero(np.diff(plan)) + 1))
    lens = np.diff(np.concatenate((starts, [plan.size])))
    return np.stack([starts + idat_start, plan[starts].astype(np.int64), lens], axis=1).astype(np.int64)


def _add_in_order(acc, src, slots, seqs):
    """acc[..., slots[i], :] += src[..., seqs[i][0], :], then seqs[i][1], ... one float32 addition at a time.  The sequences of
    different slots are independent; step k of all of them is taken at once (vectorised over slots and the leading axes)."""
    if not seqs:
        return acc
    lens = np.array([len(s) for s in seqs])
    L = int(lens.max())
    idx = np.zeros((len(seqs), L), np.int64)
    for i, s in enumerate(seqs):
        idx[i, :len(s)] = s
    slots = np.asarray(slots, np.int64)
    for k in range(L):
        m = lens > k
        sl = slots[m]
        acc[:, :, sl, :] = acc[:, :, sl, :] + src[:, :, idx[m, k], :]
    return acc


def fold_time_order(rows, runs, prof):
    """Fold.C:844-852 in float32: per (chan, pol, bin, dim) the samples of the bin's runs, in time order, added one by one to
    the profile's value."""
    rows = np.asarray(rows, np.float32)
    out = np.array(prof, np.float32, copy=True)
    per_bin = {}
    for off, b, n in np.asarray(runs, np.int64).reshape(-1, 3):
        if n:
            per_bin.setdefault(int(b), []).append(np.arange(off, off + n))
    bins = sorted(per_bin)
    return _add_in_order(out, rows, bins, [np.concatenate(per_bin[b]) for b in bins])


def long_segments(nchunk, nrow, ncu):
    """(nseg, chunks per segment) of the LONG path: fold_plan.h fold_long_segments, `nseg = (4 * ncu + nrow - 1) / nrow` ..."""
    nseg = (4 * ncu + nrow - 1) // nrow
    nseg = max(1, min(nseg, nchunk, 65535))
    cps = (nchunk + nseg - 1) // nseg
    return (nchunk + cps - 1) // cps, cps


def plan_span(runs):
    """[first, last) of the chunk grid: the plan's first sample rounded down to a multiple of 4, one past its last sample"""
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    first = int(runs[0, 0]) - int(runs[0, 0]) % 4
    return first, int(runs[-1, 0] + runs[-1, 2])


def fold_long_model(rows, runs, prof, nrow, ncu):
    """k_fold_chunked<., true, .> + k_fold_combine, bit for bit.  The chunk grid starts at plan_span's `first`, chunks of
    FOLD_CHUNK samples, grouped into nseg time segments of cps chunks (long_segments: nrow = nchan * npol, ncu = the device's
    compute units).  Every aligned FOLD_MB-sample micro-block of a chunk is summed from zero in time order.  Each segment sums
    every bin from zero: for each run piece inside a chunk, in time order, the single samples up to the first micro-block
    boundary, the whole micro-blocks, the single samples after the last boundary -- all single samples when no whole
    micro-block fits.  k_fold_combine then adds the segments' sums to the profile in segment order (every bin, every segment)."""
    rows = np.asarray(rows, np.float32)
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    out = np.array(prof, np.float32, copy=True)
    if runs.shape[0] == 0:
        return out
    nchan, npol, ndat, ndim = rows.shape
    nbin = out.shape[2]
    first, last = plan_span(runs)
    nchunk = (last - first + FOLD_CHUNK - 1) // FOLD_CHUNK
    nseg, cps = long_segments(nchunk, nrow, ncu)
    # the chunk images: samples [first, last), zero behind (the kernel's ragged-end fill)
    span = nchunk * FOLD_CHUNK
    img = np.zeros((nchan, npol, span, ndim), np.float32)
    img[:, :, :last - first, :] = rows[:, :, first:last, :]
    nmb = span // FOLD_MB
    blk = img.reshape(nchan, npol, nmb, FOLD_MB, ndim)
    mbs = np.zeros((nchan, npol, nmb, ndim), np.float32)
    for h in range(FOLD_MB):
        mbs = mbs + blk[:, :, :, h, :]
    src = np.concatenate([img, mbs], axis=2)            # term t < span: sample first + t;  span + m: micro-block m
    seqs = {}
    for off, b, n in runs:
        s, e = int(off) - first, int(off + n) - first
        while s < e:
            c = s // FOLD_CHUNK
            c0 = c * FOLD_CHUNK
            hi = min(e, c0 + FOLD_CHUNK)
            s0, s1 = s - c0, hi - c0
            a0 = -(-s0 // FOLD_MB) * FOLD_MB
            a1 = s1 // FOLD_MB * FOLD_MB
            if a0 >= a1:
                t = list(range(c0 + s0, c0 + s1))
            else:
                t = (list(range(c0 + s0, c0 + a0)) + [span + (c0 + a) // FOLD_MB for a in range(a0, a1, FOLD_MB)]
                     + list(range(c0 + a1, c0 + s1)))
            seqs.setdefault((c // cps, int(b)), []).extend(t)
            s = hi
    part = np.zeros((nchan, npol, nseg * nbin, ndim), np.float32)
    keys = sorted(seqs)
    _add_in_order(part, src, [g * nbin + b for g, b in keys], [seqs[k] for k in keys])
    for g in range(nseg):
        out = out + part[:, :, g * nbin:(g + 1) * nbin, :]
    return out


def fold_dispatch(addr, chan_stride, pol_stride, nchan, npol, ndim, nbin, runs, ncu):
    """fold_plan.h fold_shape's choice for a call of dspsr_amd_fold_fold (the comments name the rules; plan_scan is fold_plan.h's too): `addr` the
    input's byte address, strides in floats.  Returns a dict:
    kernel ('direct' | 'chunked' | 'long' | 'dense'), ndim, nrow (NROW), nsplit (exact kernels, grid.z), nseg and cps (LONG),
    threads."""
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    first, last = plan_span(runs)
    aligned = addr % 16 == 0 and chan_stride % 4 == 0 and pol_stride % 4 == 0                      # `aligned`
    fits = nbin <= FOLD_BPT * 1024
    nchunk = (last - first + FOLD_CHUNK - 1) // FOLD_CHUNK
    one_per_chunk = aligned and fits                                                                 # plan_scan: the table's size
    if one_per_chunk:
        ntab = nchunk * nbin
        one_per_chunk = ntab <= (1 << 24) and 4 * ntab <= (last - first) * nchan * npol * ndim
    if one_per_chunk:                                                                                # plan_scan: the walk
        lastc = {}
        for off, b, n in runs:
            if n == 0:
                continue
            c0, c1 = (off - first) // FOLD_CHUNK, (off - first + n - 1) // FOLD_CHUNK
            if lastc.get(int(b)) == c0:
                one_per_chunk = False
                break
            lastc[int(b)] = c1
    max_run = int(runs[:, 2].max())
    lng = aligned and fits and max_run >= FOLD_LONG_RUN                                              # `lng`
    dense = one_per_chunk and not lng
    nrow_all = nchan * npol
    nsplit = 1
    if not lng:                                                                                      # `nsplit`
        while nsplit < 8 and nrow_all * nsplit < 512 and nbin // (2 * nsplit) >= 64:
            nsplit *= 2
    threads = ((nbin + 63) // 64) * 64 if nbin < 1024 else 1024
    if not (aligned and fits):                                                                       # k_fold_direct
        return dict(kernel="direct", ndim=ndim, nrow=1, nsplit=nsplit, nseg=1, cps=nchunk, threads=threads)
    bins_wg = (nbin + nsplit - 1) // nsplit                                                          # `threads`
    threads = min(1024, max(256, ((bins_wg + FOLD_BPT - 1) // FOLD_BPT + 63) // 64 * 64))
    nseg, cps = long_segments(nchunk, nrow_all, ncu) if lng else (1, nchunk)                         # `nseg`, `cps`
    nrw = npol if (ndim * npol == 4 and ndim < 4 and nchan * (nseg if lng else nsplit) >= 2 * ncu) else 1   # `nrw`
    kernel = "dense" if dense else ("long" if lng else "chunked")
    return dict(kernel=kernel, ndim=ndim, nrow=nrw, nsplit=1 if lng else nsplit, nseg=nseg, cps=cps, threads=threads)


def fold_many_dispatch(nchan, npol, ndim, nslot, ncu):
    """fold_plan.h fold_many_shape: one launch of k_fold_many over nslot (plan, bin) slots.  Returns a dict: nz (workgroups per
    row, grid.x), threads, nrow (NROW)."""
    nz = 1
    while nz * FOLD_BPT * FOLD_MANY_THREADS < nslot:                                                 # FOLD_BPT slots per thread
        nz *= 2
    while nz < 8 and nchan * npol * nz < 512 and nslot // (2 * nz) >= 64:                           # fold_bin_split
        nz *= 2
    slots_wg = (nslot + nz - 1) // nz
    threads = min(FOLD_MANY_THREADS, max(256, ((slots_wg + FOLD_BPT - 1) // FOLD_BPT + 63) // 64 * 64))
    nrw = npol if (ndim * npol == 4 and ndim < 4 and nchan * nz >= 2 * ncu) else 1
    return dict(nz=nz, threads=threads, nrow=nrw)


# ---- the fold inside the last filterbank pass (k_inv_chan<., FOLD>, k_rows_inv<., ., FOLD>) ------------------------------------
FUSED_MAX_SEG = 16       # runs of a segmented launch at most (filterbank.hip fb_launch_fused: `if (nseg > 16) nseg = 16`)


def fused_nseg(ns, tiles, wgs):
    """fb_launch_fused's number of runs for a segmented launch of `ns` parts: clamp(wgs / tiles, 1, min(ns, 16)), one when the
    tiles fill the workgroups (`segmented && tiles < wgs`)"""
    if tiles >= wgs:
        return 1
    return max(1, min(wgs // tiles, ns, FUSED_MAX_SEG))


def fused_runs_of_launch(ns, nseg):
    """the kernel's run arithmetic (fb_inv_walk.h: pps, p0, np): [(first part, parts)] of runs 0 .. nseg - 1 of a launch of
    ns parts; trailing runs may hold no part (their workgroups return at once)"""
    fpps = -(-ns // nseg)
    return [(s * fpps, max(0, min(ns, (s + 1) * fpps) - s * fpps)) for s in range(nseg)]


def clip_runs(runs, first, last):
    """the pieces of the plan's runs inside samples [first, last)"""
    out = []
    for off, b, n in np.asarray(runs, np.int64).reshape(-1, 3):
        lo, hi = max(int(off), first), min(int(off + n), last)
        if hi > lo:
            out.append((lo, int(b), hi - lo))
    return np.array(out, np.int64).reshape(-1, 3)


def fused_launch_sums(rows, runs, out, nkeep, part0, ns, nseg):
    """One launch of ns parts from part part0 of the call, cut into nseg runs: (`out` with run 0 added in time order, the sums
    from zero of runs 1 .. nseg - 1 in time order); rows [chan][1][ndat][4], out [chan][1][nbin][4]"""
    partial = []
    for s, (p0, np_) in enumerate(fused_runs_of_launch(ns, nseg)):
        piece = clip_runs(runs, (part0 + p0) * nkeep, (part0 + p0 + np_) * nkeep)
        if s == 0:
            out = fold_time_order(rows, piece, out)
        else:
            partial.append(fold_time_order(rows, piece, np.zeros_like(out)))
    return out, partial


def fused_fold_model(det, runs, profile, nkeep, launches, mode, nseg_of=None):
    """The profile after dspsr_amd_filterbank_perform_fold of one call, bit for bit.  det: the detected samples float32
    [chan][ndat][4] of the call (ndat = parts * nkeep); runs: the call's plan; profile: [chan][npol][nbin][ndim] with
    npol * ndim = 4 (a bin's four sums are independent: the 2 x 2 profile holds the same bits in another place); launches: the
    parts of every launch of the fused kernel, in order (fb_group_parts: min(left, max_parts) while the passes stay below 2^31
    items); mode = fold_is_fused().
      mode 1: every (chan, bin) sum in strict time order onto the profile -- a launch walks its parts in order, launches are
              stream ordered: fold_time_order of the whole call.
      mode 2: the ns parts of a launch are cut into nseg_of(ns) runs (fused_runs_of_launch); run 0 adds onto the profile in
              time order, every other run sums from zero in time order, and k_fold_combine adds those sums to the profile in
              run order, every bin of every run: profile = ((profile + p1) + p2) + ..."""
    det = np.asarray(det, np.float32)
    rows = det[:, None, :, :]
    shape = np.shape(profile)
    nchan, nbin = shape[0], shape[2]
    assert shape[1] * shape[3] == 4 and det.shape[0] == nchan and det.shape[2] == 4
    # (chan, pol, bin, dim) -> (chan, 1, bin, 2 * pol + dim): the float4 the kernel keeps per (chan, bin)
    out = np.array(profile, np.float32).transpose(0, 2, 1, 3).reshape(nchan, 1, nbin, 4)
    assert mode in (1, 2)
    part0 = 0
    for ns in launches:
        out, partial = fused_launch_sums(rows, runs, out, nkeep, part0, ns, 1 if mode == 1 else nseg_of(ns))
        for p in partial:
            out = out + p
        part0 += ns
    assert part0 * nkeep == det.shape[1], "the launches do not cover the call"
    return out.reshape(nchan, nbin, shape[1], shape[3]).transpose(0, 2, 1, 3)
