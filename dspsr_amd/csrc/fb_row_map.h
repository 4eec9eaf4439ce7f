// Mirror-paired row order of the scratch array A and of the pass-2 tiles (pre-split spectrum): integer
// arithmetic only, standard headers only, shared by the kernels (k_fwd_cols copy-out, k_fwd_rows), the host dispatch and
// tests/row_map_driver.cpp, which runs it without a GPU.
//
// Pass 1 leaves rows ka < M = 2^logM of A; a pass-2 tile holds T2 = 2^logT2 of them (1 <= logT2 <= logM), one block
// A[block][nb][r].  The Hermitian split of real dual-polarisation input pairs spectrum element (row m, channel c) with
// (row M - m, channel Rr - 1 - c): pass 2 can only form it inside its tile when the tile holds every row together with its mirror.
// With h = T2 / 2, block j holds
//   r <  h : row  h j + r                       (ascending)
//   r >= h : row  M - (h j + (r - h))           (the mirrors, descending), but row M / 2 for j = 0, r = h
// Rows 0 and M / 2 are their own mirrors and sit in block 0, slots 0 and h.  The mirror of slot r is slot r ^ h of the same block.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RM_HD __host__ __device__ inline
#else
#define RM_HD inline
#endif

namespace dspsr_amd {

struct RowSlot { uint32_t block, r; };

// row ka held by slot r of block `block`
RM_HD uint32_t rm_row(const int logM, const int logT2, const uint32_t block, const uint32_t r)
{
  const uint32_t h = 1u << (logT2 - 1);
  const uint32_t m = (block << (logT2 - 1)) + (r & (h - 1));       // < M / 2
  if (r < h) return m;
  return m ? (1u << logM) - m : 1u << (logM - 1);
}

// (block, slot) of row ka
RM_HD RowSlot rm_slot(const int logM, const int logT2, const uint32_t ka)
{
  const uint32_t h = 1u << (logT2 - 1), half = 1u << (logM - 1);
  RowSlot s;
  if (ka < half) { s.block = ka >> (logT2 - 1); s.r = ka & (h - 1); return s; }
  const uint32_t m = ((1u << logM) - ka) & (half - 1);             // M / 2 -> 0
  s.block = m >> (logT2 - 1);
  s.r = h + (m & (h - 1));
  return s;
}

// slot of the same block that holds row (M - ka) mod M, ka the row of slot r
RM_HD uint32_t rm_mirror(const int logT2, const uint32_t block, const uint32_t r)
{
  const uint32_t h = 1u << (logT2 - 1);
  return (block == 0 && (r & (h - 1)) == 0) ? r : r ^ h;
}

// Pre-split spectrum X' (same size as X): the two polarisations (x0, x1) of channel c < C, bin m as one 16-byte element at index
// ((c >> logX3) * M + p(m)) << logX3 | c % X3 -- the X layout with 16-byte elements and the bins above M / 2 moved down by one
// place, bin M / 2 taking the last: p(m) = m for m < M / 2, m - 1 for m > M / 2, M - 1 for m = M / 2.  The upper half of block j
// is the rows M - h j - (h - 1) .. M - h j, one past a multiple of h: in their own places the h * X3 elements a pass-2 tile
// stores per channel block would straddle two aligned runs, each shared with the neighbouring tile (measured: pass 2 +30 %,
// profiles/r07_experiments.txt item 2); moved down by one they are ONE aligned run, like the lower half's.
RM_HD uint32_t rm_xrow(const int logM, const uint32_t m)
{
  const uint32_t half = 1u << (logM - 1);
  return m < half ? m : m == half ? (1u << logM) - 1 : m - 1;
}
RM_HD uint64_t rm_xsplit_index(const int logM, const int logX3, const uint32_t c, const uint32_t m)
{
  return ((((uint64_t)(c >> logX3) << logM) + rm_xrow(logM, m)) << logX3) | (c & ((1u << logX3) - 1));
}

}  // namespace dspsr_amd
