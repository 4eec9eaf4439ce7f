// Work items of the inverse passes k_inv_chan (fb_inv_chan.h) and k_rows_inv (fb_two_pass.hip): which (tile of channels, part of the
// launch) workgroup b of a persistent grid takes as its item jj.  Integer arithmetic only, standard headers only; the workgroup index
// and the grid size are arguments, so tests/inv_walk_driver.cpp runs the same text without a GPU.
//
// A work item is kept as two 32-bit numbers: a combined 64-bit index costs a software 64-bit division per use (about 300 scalar
// instructions per tile in the r02c listing).
//
// Ordered (the fused fold and search mode, EPI != 0): a workgroup walks the parts of ITS tile in order -- the fold's profile and the
// scrunch's carry are sums in time order -- and takes tiles lane, lane + ntg, ...
//   Segmented (fused fold with nseg > 1, geometries with fewer channel tiles than compute units; host: grid % nseg == 0): the parts of
//   the launch are cut into nseg runs of pps parts; workgroup (lane, seg) walks the parts [p0, p0 + np) of run `seg` for tiles lane,
//   lane + ntg, ...  Run 0 adds onto the profile (it continues the sums of earlier launches in time order), the others onto zeroed
//   partial profiles that are added to the profile, in run order, after the launch -- the sums of a launch are re-associated per run.
//   xcd_lr > 0 (k_inv_chan's fused fold alone, lr = logX3 - logT3): tiles that share an X layout block (2^lr of them) go to workgroups
//   b, b + 8, ...: one XCD under the observed round-robin placement, at the same time, so the block's lines are fetched once (speed
//   only: a permutation of the lanes).
// Free order (EPI == 0): when every workgroup gets the same number of tiles it also walks the parts of a tile one after the other, so
// that the tile's chirp stays in registers (one chirp read per launch, not per part); otherwise the items are dealt XCD-wise as in
// the other passes, part fastest, so one XCD re-reads a tile's chirp rows from its L2 for every part.
//   matrix (the Jones-matrix forms of k_inv_chan): tile after tile whenever the tiles alone occupy every workgroup, also with a
//   remainder -- the response is re-read per part, from the cache while the tile's rows are warm; fewer tiles than workgroups keep the
//   XCD dealing.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IW_HD __host__ __device__ __forceinline__
#else
#define IW_HD inline
#endif

namespace dspsr_amd {

struct InvItem { uint32_t tile, lp; };

struct InvWalk {
  uint32_t wg, grid;               // this workgroup, workgroups of the launch
  uint32_t lane, ntg;              // tile-major: this workgroup's tiles are lane, lane + ntg, ... (ntg = workgroups per run)
  uint32_t seg, pps, p0, np;       // run of parts this workgroup walks: run `seg` of pps parts, [p0, p0 + np) of the launch
  uint32_t nparts, ntile, run;
  bool tile_major;
};

// nseg: runs of a segmented fused fold, otherwise 1.  np == 0 (a run behind the launch's last part): the workgroup has no item.
IW_HD InvWalk inv_walk(const bool ordered, const bool matrix, const uint32_t nseg, const uint32_t nparts, const uint32_t ntile,
                       const uint32_t run, const uint32_t grid, const uint32_t b, const int xcd_lr)
{
  InvWalk w;
  w.wg = b; w.grid = grid; w.nparts = nparts; w.ntile = ntile; w.run = run;
  const uint32_t ns = nseg > 1 ? nseg : 1u;
  w.ntg = grid / ns;
  w.seg = ns > 1 ? b / w.ntg : 0u;
  w.pps = (nparts + ns - 1) / ns;
  w.p0 = w.seg * w.pps;
  w.np = w.p0 >= nparts ? 0u : (nparts - w.p0 < w.pps ? nparts - w.p0 : w.pps);
  w.lane = b - w.seg * w.ntg;
  if (ns == 1 && xcd_lr > 0 && (grid & ((8u << xcd_lr) - 1)) == 0)
    w.lane = ((((b >> (3 + xcd_lr)) << 3) | (b & 7)) << xcd_lr) | ((b >> 3) & ((1u << xcd_lr) - 1));
  w.tile_major = ordered || (ntile >= grid && (matrix || ntile % grid == 0));
  return w;
}

// item jj of the workgroup, or false: none, and none behind it
IW_HD bool inv_walk_item(const InvWalk& w, const uint32_t jj, InvItem& it)
{
  if (w.tile_major) {
    const uint32_t q = jj / w.np;                      // (32-bit; jj counts this workgroup's items)
    it.tile = w.lane + q * w.ntg;
    it.lp = w.p0 + (jj - q * w.np);
    return it.tile < w.ntile;
  }
  // XCD dealing as persistent_item (wgfft.h) with runs of `run` items; run == nparts (the default) makes the run index the tile and
  // the position in the run the part, without a division by nparts
  uint32_t hi, lo;
  if (w.grid & 7) {
    const uint32_t lin = w.wg + jj * w.grid;
    hi = lin / w.run; lo = lin - hi * w.run;
  } else {
    const uint32_t q = jj * (w.grid >> 3) + (w.wg >> 3);
    const uint32_t qr = q / w.run;
    hi = qr * 8 + (w.wg & 7); lo = q - qr * w.run;
  }
  if (w.run == w.nparts) { it.tile = hi; it.lp = lo; }
  else { const uint32_t lin = hi * w.run + lo; it.tile = lin / w.nparts; it.lp = lin - it.tile * w.nparts; }
  return it.tile < w.ntile;                            // (lp < nparts by construction)
}

}  // namespace dspsr_amd
