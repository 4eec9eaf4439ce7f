// The fold engine's plan builders and launch shapes: integer arithmetic on the run-length plan and on the call's dimensions,
// standard headers only (tests/fold_plan_driver.cpp runs them without a GPU).  Each builder writes straight into the pointers it is given -- the pinned buffers of a PlanSlot -- with
// `cursor` (dspsr_amd_fold::cursor) as its only scratch.  This code runs once per block next to a kernel of a few hundred
// microseconds; extra walks and a bucket sort nobody read once made the host as slow as the device (profiles/r05_experiments.txt 6).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

namespace dspsr_amd {
struct Interval { uint64_t offset; uint32_t hits; uint32_t pad; };   // sorted by (bin, time)
struct RunBin { uint32_t ibin, hits; uint64_t offset; };             // FoldCUDA.h:19-24

// What the host's plans and the kernels' walks must agree on.
constexpr uint32_t FOLD_CHUNK = 2048;   // samples per chunk of the chunked / dense / many kernels (fold.hip)
// Runs of FOLD_LONG_RUN samples or more are folded with re-associated sums (fold.hip, k_fold_chunked<., true>); the fused
// filterbank kernel only has the exact time-order fold, so such plans take the separate Detection + Fold launches.
constexpr uint32_t FOLD_LONG_RUN = 64;
constexpr uint32_t FOLD_BPT = 4;        // bins per thread of those kernels (nbin <= FOLD_BPT * blockDim)
constexpr uint32_t FOLD_MB = 32;        // samples per micro-block of the LONG association (fold.hip, "LONG runs")
constexpr uint32_t FOLD_MANY_THREADS = 512;   // threads per workgroup of k_fold_many, at most (fold.hip)

// Longest run of a plan (samples that go to one phase bin in a row); open_hits: the samples of the last run while it is
// still open (its own hits are final only once the plan is closed).
inline uint32_t plan_max_run(const RunBin* runs, size_t n, uint32_t open_hits)
{
  uint32_t m = open_hits;
  for (size_t i = 0; i < n; i++) if (runs[i].hits > m) m = runs[i].hits;
  return m;
}

// One walk over the runs of a closed plan decides which kernel folds them: the longest run (the return value; see
// FOLD_LONG_RUN) and, when try_dense, whether the plan fits the dense per-chunk table of k_fold_dense over the chunk grid that
// starts at `first` -- at most one run per (chunk, phase bin), runs cut at the chunk ends; a plan with two runs of a bin inside
// a chunk (a folding period shorter than the chunk) does not.  The table (*ntab words) is also refused beyond 2^24 entries and
// when it would be more than a quarter of the words it helps to fold (few channels, many bins); row_words = nchan * npol * ndim.
inline uint32_t plan_scan(const RunBin* runs, size_t n, uint32_t nbin, uint64_t row_words, bool try_dense, uint64_t first,
                          uint64_t last, std::vector<uint32_t>& cursor, size_t* ntab, bool* one_per_chunk)
{
  uint32_t max_run = 0;
  bool ok = try_dense;
  *ntab = 0;
  if (ok) {
    const uint64_t nchunk = (last - first + FOLD_CHUNK - 1) / FOLD_CHUNK;
    *ntab = (size_t)nchunk * nbin;
    ok = *ntab <= ((size_t)1 << 24) && 4 * (uint64_t)*ntab <= (last - first) * row_words;
  }
  if (ok) {
    cursor.assign(nbin, ~0u);                               // (scratch: chunk of the bin's previous piece)
    uint32_t* const lastc = cursor.data();
    for (size_t i = 0; i < n; i++) {
      const RunBin& r = runs[i];
      if (r.hits > max_run) max_run = r.hits;
      if (r.hits == 0 || !ok) continue;
      const uint64_t c0 = (r.offset - first) / FOLD_CHUNK, c1 = (r.offset - first + r.hits - 1) / FOLD_CHUNK;
      if (lastc[r.ibin] == (uint32_t)c0) ok = false;                       // a second run of this bin in the chunk
      lastc[r.ibin] = (uint32_t)c1;
    }
  } else {
    max_run = plan_max_run(runs, n, 0);
  }
  *one_per_chunk = ok;
  return max_run;
}

// The runs as intervals bucketed by phase bin (stable => time order kept inside a bin): bin_start[0 .. nbin], iv[0 .. n).
// What the walk kernels and the per-channel hit count of a zeroed input read -- not the dense kernel.
inline void plan_bucket(const RunBin* runs, size_t n, uint32_t nbin, uint32_t* bin_start, Interval* iv, std::vector<uint32_t>& cursor)
{
  for (uint32_t b = 0; b <= nbin; b++) bin_start[b] = 0;
  for (size_t i = 0; i < n; i++) bin_start[runs[i].ibin + 1]++;
  for (uint32_t b = 0; b < nbin; b++) bin_start[b + 1] += bin_start[b];
  cursor.assign(bin_start, bin_start + nbin);
  for (size_t i = 0; i < n; i++) {
    Interval v; v.offset = runs[i].offset; v.hits = runs[i].hits; v.pad = 0;
    iv[cursor[runs[i].ibin]++] = v;
  }
}

// The dense table tab[chunk][bin] = first sample of the run inside the chunk | samples << 11 (0: none) over the chunk grid
// that starts at `first`; ntab as plan_scan gave it for a plan it accepted.
inline void plan_dense_fill(const RunBin* runs, size_t n, uint32_t nbin, uint64_t first, uint32_t* tab, size_t ntab)
{
  ::memset((void*)tab, 0, ntab * sizeof(uint32_t));
  for (size_t i = 0; i < n; i++) {
    uint64_t off = runs[i].offset - first;
    uint32_t left = runs[i].hits;
    while (left) {
      const uint64_t c = off / FOLD_CHUNK;
      const uint32_t s0 = (uint32_t)(off % FOLD_CHUNK), m = left < FOLD_CHUNK - s0 ? left : FOLD_CHUNK - s0;
      tab[c * nbin + runs[i].ibin] = s0 | (m << 11);
      off += m;
      left -= m;
    }
  }
}

// Part plan of the fused fold (fb_inv_chan.h): the runs cut at every multiple of nkeep, the pieces bucketed by (part, bin),
// offsets relative to the start of the part.  One uint32 array + the interval array:
//   start[0 .. npart]                   first active-bin entry of every part (start[npart] = total)
//   start[align4(npart+1) + 4*e + 0..3]  entry e = { bin, first interval, count << 16 | hits0, offset0 }, 16-byte aligned
// Only the phase bins that receive samples in a part are listed, so a workgroup finds its work with two dependent loads
// (entry, then interval + accumulator) instead of walking all nbin bins.  nkeep must be < 65536.
// In two steps, because the buffers are sized between them.
struct PartPlanSize { size_t npiece, nentry, nwords; };
template <class Fn>
inline void part_plan_pieces(const RunBin* runs, size_t n, uint32_t nkeep, Fn&& fn)
{
  for (size_t i = 0; i < n; i++) {
    uint64_t off = runs[i].offset, left = runs[i].hits;
    while (left) {
      const uint64_t part = off / nkeep, within = off % nkeep;
      const uint64_t m = left < nkeep - within ? left : nkeep - within;
      fn((uint32_t)part, runs[i].ibin, within, (uint32_t)m);
      off += m; left -= m;
    }
  }
}
inline size_t part_plan_entry_offset(uint32_t npart) { return ((size_t)npart + 1 + 3) & ~(size_t)3; }
// false: *beyond is a plan sample behind the npart parts.  Leaves in `cursor` the first interval of every (part, bin) bucket.
inline bool part_plan_count(const RunBin* runs, size_t n, uint32_t nkeep, uint32_t npart, uint32_t nbin, std::vector<uint32_t>& cursor,
                            PartPlanSize* size, uint64_t* beyond)
{
  size_t npiece = 0;
  for (size_t i = 0; i < n; i++) {
    if (!runs[i].hits) continue;
    const uint64_t p0 = runs[i].offset / nkeep, p1 = (runs[i].offset + runs[i].hits - 1) / nkeep;
    if (p1 >= npart) { *beyond = runs[i].offset + runs[i].hits - 1; return false; }
    npiece += (size_t)(p1 - p0 + 1);
  }
  const size_t nb1 = (size_t)npart * nbin;
  cursor.assign(nb1 + 1, 0u);
  uint32_t* const cnt = cursor.data();
  part_plan_pieces(runs, n, nkeep, [&](uint32_t part, uint32_t ibin, uint64_t, uint32_t) { cnt[(size_t)part * nbin + ibin + 1]++; });
  size_t nentry = 0;
  for (size_t i = 0; i < nb1; i++) { if (cnt[i + 1]) nentry++; cnt[i + 1] += cnt[i]; }
  size->npiece = npiece;
  size->nentry = nentry;
  size->nwords = part_plan_entry_offset(npart) + 4 * nentry;
  return true;
}
// start: size.nwords words, iv: size.npiece intervals; `cursor` as part_plan_count left it
inline void part_plan_fill(const RunBin* runs, size_t n, uint32_t nkeep, uint32_t npart, uint32_t nbin, std::vector<uint32_t>& cursor,
                           uint32_t* start, Interval* iv)
{
  // the fill moves every bucket's cursor to its end, the first interval of the next bucket: bucket i is iv[end[i-1] .. end[i])
  uint32_t* const end = cursor.data();
  part_plan_pieces(runs, n, nkeep, [&](uint32_t part, uint32_t ibin, uint64_t within, uint32_t m) {
    Interval v; v.offset = within; v.hits = m; v.pad = 0;
    iv[end[(size_t)part * nbin + ibin]++] = v;
  });
  const size_t ent_off = part_plan_entry_offset(npart);
  uint32_t* ent = start + ent_off;
  for (size_t i = (size_t)npart + 1; i < ent_off; i++) start[i] = 0;
  size_t e = 0;
  uint32_t i0 = 0;
  for (uint32_t part = 0; part < npart; part++) {
    start[part] = (uint32_t)e;
    for (uint32_t b = 0; b < nbin; b++) {
      const uint32_t i1 = end[(size_t)part * nbin + b], m = i1 - i0;
      if (m) {
        // count, hits and offsets are < nkeep <= 8192 on the three-pass path
        ent[4 * e] = b; ent[4 * e + 1] = i0; ent[4 * e + 2] = (m << 16) | iv[i0].hits; ent[4 * e + 3] = (uint32_t)iv[i0].offset;
        e++;
      }
      i0 = i1;
    }
  }
  start[npart] = (uint32_t)e;
}

// Segment plan of the four-pass fused fold (fb_four_pass.hip k_inv_b<., true>): the plan must cover samples [0, ndat) without
// gaps, ndat < 2^32, and every interval but the first and the last must hold at least `seg` samples (so that a `seg`-sample
// run of the last inverse pass is cut by at most one phase-bin boundary).  The plan may still be open: open_hits stands for
// the last run's hits when it is not zero.
inline bool segment_plan_qualifies(const RunBin* runs, size_t n, uint32_t open_hits, uint64_t ndat, uint32_t seg)
{
  if (n == 0 || ndat == 0 || ndat >= (1ull << 32)) return false;
  uint64_t expect = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t h = i + 1 == n && open_hits ? open_hits : runs[i].hits;
    if (runs[i].offset != expect || h == 0) return false;                  // a gap (dropped samples) or an offset start
    if (i > 0 && i + 1 < n && h < seg) return false;                       // an inner interval shorter than a segment
    expect += h;
  }
  return expect == ndat;
}
inline size_t segment_plan_nblk(uint64_t ndat) { return (size_t)(ndat >> 10) + 1; }
//   run_off[0 .. n]                        start offsets of the time-ordered intervals, run_off[n] = ndat
//   blk_first[0 .. segment_plan_nblk)      index of the interval that holds sample 1024 * i
//   bin_start / iv                         plan_bucket of the same runs
inline void segment_plan_fill(const RunBin* runs, size_t n, uint32_t nbin, uint64_t ndat, uint32_t* run_off, uint32_t* blk_first,
                              uint32_t* bin_start, Interval* iv, std::vector<uint32_t>& cursor)
{
  for (size_t i = 0; i < n; i++) run_off[i] = (uint32_t)runs[i].offset;
  run_off[n] = (uint32_t)ndat;
  const size_t nblk = segment_plan_nblk(ndat);
  size_t q = 0;
  for (size_t i = 0; i < nblk; i++) {
    const uint64_t s0 = (uint64_t)i << 10;
    while (q + 1 < n && run_off[q + 1] <= s0) q++;
    blk_first[i] = (uint32_t)q;
  }
  plan_bucket(runs, n, nbin, bin_start, iv, cursor);
}

// ---- launch shapes: which kernel folds a call, and over which grid.  Each rule once, then one function per entry point. ---------

// the chunk kernels take 16-byte aligned rows and at most FOLD_BPT bins per thread of a 1024-thread workgroup; else k_fold_direct
inline bool fold_takes_chunks(bool aligned, uint32_t nbin) { return aligned && nbin <= FOLD_BPT * 1024; }

// Exact order: the bins (slots) of a row are dealt to n workgroups, from `n` on doubled until there are two workgroups per CU
// -- when the band has few rows -- or eight per row, or fewer than 64 bins each
inline uint32_t fold_bin_split(uint64_t nrow, uint32_t nbin, uint32_t n)
{
  while (n < 8 && nrow * n < 512 && nbin / (2 * n) >= 64) n *= 2;
  return n;
}

// FOLD_BPT bins per thread: 256-thread workgroups for 1024 bins or fewer, so that four of them share a CU and keep 4 x 32 KiB of
// chunk loads in flight (the kernels are HBM-latency bound per workgroup)
inline uint32_t fold_threads(uint32_t bins_wg, uint32_t max_threads)
{
  const uint32_t t = ((bins_wg + FOLD_BPT - 1) / FOLD_BPT + 63) / 64 * 64;
  return t < 256 ? 256 : t > max_threads ? max_threads : t;
}

// LONG: rows x time segments, about four workgroups per CU, every sample read once.  nunit >= 1 units (chunks) of the span are
// dealt to nseg segments of `len` units, the last one maybe shorter.
struct FoldSegments { uint32_t nseg; uint64_t len; };
inline FoldSegments fold_long_segments(uint64_t nunit, uint64_t nrow, uint32_t ncu)
{
  uint64_t nseg = (4ull * ncu + nrow - 1) / nrow;
  if (nseg > nunit) nseg = nunit;
  if (nseg > 65535) nseg = 65535;
  if (nseg < 1) nseg = 1;
  FoldSegments s;
  s.len = (nunit + nseg - 1) / nseg;
  s.nseg = (uint32_t)((nunit + s.len - 1) / s.len);
  return s;
}

// planes of one channel folded together (ndim < 4): 4 or 2 rows per workgroup when the channels alone fill the chip, nz
// workgroups per row (one row per workgroup at Benchmark/fold.csh's shape, four times the workgroups: 311-313 against 321-331
// Msamples/s, same box)
inline uint32_t fold_rows_per_wg(uint32_t nchan, uint32_t npol, uint32_t ndim, uint64_t nz, uint32_t ncu)
{
  return (ndim * npol == 4 && ndim < 4 && nchan * nz >= 2ull * ncu) ? npol : 1u;
}

enum FoldFamily { FOLD_DIRECT, FOLD_CHUNKED, FOLD_LONG, FOLD_DENSE, FOLD_MANY, FOLD_MOMENTS, FOLD_MOMENTS_LONG };
struct FoldShape {
  FoldFamily family;
  uint32_t nd, nr;         // the instantiation <ND, NR>: floats per sample, rows per workgroup
  uint32_t grid[3], threads;
  size_t lds;              // dynamic LDS bytes
  uint32_t nseg;           // LONG: time segments (else 1) of ...
  uint64_t seg_len;        // ... this many chunks (fold) or samples (moments) each
};

// dspsr_amd_fold_fold: the plan spans samples [first, last), its longest run is max_run, `dense`: plan_scan accepted the table
inline FoldShape fold_shape(bool aligned, uint32_t nchan, uint32_t npol, uint32_t ndim, uint32_t nbin, uint64_t first, uint64_t last,
                            uint32_t max_run, bool dense, uint32_t ncu)
{
  const bool chunked = fold_takes_chunks(aligned, nbin);
  const bool lng = chunked && max_run >= FOLD_LONG_RUN;               // re-associated sums (see FOLD_LONG_RUN)
  const uint64_t nrow = (uint64_t)npol * nchan;
  const uint32_t nsplit = lng ? 1u : fold_bin_split(nrow, nbin, 1);
  const uint64_t nchunk = (last - first + FOLD_CHUNK - 1) / FOLD_CHUNK;
  FoldShape s;
  s.nd = ndim;
  s.nseg = 1;
  s.seg_len = nchunk;
  if (!chunked) {
    s.family = FOLD_DIRECT;
    s.nr = 1;
    s.grid[0] = npol; s.grid[1] = nchan; s.grid[2] = nsplit;
    s.threads = nbin < 1024 ? ((nbin + 63) / 64) * 64 : 1024;
    s.lds = 0;
    return s;
  }
  if (lng) {
    const FoldSegments g = fold_long_segments(nchunk, nrow, ncu);
    s.nseg = g.nseg;
    s.seg_len = g.len;
  }
  const uint32_t nz = lng ? s.nseg : nsplit;
  s.family = dense ? FOLD_DENSE : lng ? FOLD_LONG : FOLD_CHUNKED;
  s.nr = fold_rows_per_wg(nchan, npol, ndim, nz, ncu);
  s.grid[0] = npol / s.nr; s.grid[1] = nchan; s.grid[2] = nz;
  s.threads = fold_threads((nbin + nsplit - 1) / nsplit, 1024);
  s.lds = ((size_t)FOLD_CHUNK + (lng ? FOLD_CHUNK / FOLD_MB : 0)) * ndim * s.nr * sizeof(float);
  return s;
}

// One launch of k_fold_many over nslot (plan, bin) slots: the slots of a row dealt to grid[0] workgroups, enough for FOLD_BPT
// slots per thread, then as fold_bin_split.  Siblings of a row are neighbours in blockIdx.x and run at the same time, so that the
// re-reads of its chunks come from the Infinity Cache.
inline FoldShape fold_many_shape(uint32_t nchan, uint32_t npol, uint32_t ndim, uint32_t nslot, uint32_t ncu)
{
  uint32_t nz = 1;
  while ((uint64_t)nz * FOLD_BPT * FOLD_MANY_THREADS < nslot) nz *= 2;
  nz = fold_bin_split((uint64_t)npol * nchan, nslot, nz);
  FoldShape s;
  s.family = FOLD_MANY;
  s.nd = ndim;
  s.nr = fold_rows_per_wg(nchan, npol, ndim, nz, ncu);
  s.grid[0] = nz; s.grid[1] = npol / s.nr; s.grid[2] = nchan;
  s.threads = fold_threads((nslot + nz - 1) / nz, FOLD_MANY_THREADS);
  s.lds = (size_t)FOLD_CHUNK * ndim * s.nr * sizeof(float);
  s.nseg = 1;
  s.seg_len = 0;
  return s;
}

// k_fold_moments (fold_moments.hip: workgroups of `threads` threads, bins_wg bins each, ndim floats per folded sample), either
// loader: bin groups (grid[0]) enough for bins_wg bins each, more as fold_bin_split when the band has few channels; LONG: time
// segments of whole FOLD_CHUNK-sample units (both loaders' chunk grids nest in them)
inline FoldShape fold_moments_shape(uint32_t nchan, uint32_t nbin, uint64_t first, uint64_t last, uint32_t max_run, uint32_t ncu,
                                    uint32_t ndim, uint32_t threads, uint32_t bins_wg)
{
  const bool lng = max_run >= FOLD_LONG_RUN;
  uint32_t ngroup = (nbin + bins_wg - 1) / bins_wg;
  if (!lng) ngroup = fold_bin_split(nchan, nbin, ngroup);
  const uint64_t nunit = (last - first + FOLD_CHUNK - 1) / FOLD_CHUNK;
  FoldSegments g = {1u, nunit};
  if (lng) g = fold_long_segments(nunit, (uint64_t)nchan * ngroup, ncu);
  FoldShape s;
  s.family = lng ? FOLD_MOMENTS_LONG : FOLD_MOMENTS;
  s.nd = ndim;
  s.nr = 1;
  s.grid[0] = ngroup; s.grid[1] = nchan; s.grid[2] = g.nseg;
  s.threads = threads;
  s.lds = 0;
  s.nseg = g.nseg;
  s.seg_len = g.len * FOLD_CHUNK;
  return s;
}
}  // namespace dspsr_amd
