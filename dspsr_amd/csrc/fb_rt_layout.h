// Layout of the regrouped input of pass 1 (k_raw_transpose / k_float_transpose -> k_fwd_cols): integer arithmetic only, standard
// headers only, shared by the kernels, the host dispatch (filterbank.hip) and tests/rt_layout_driver.cpp, which runs it without a GPU.
//
// A row is the Rr = 2^logR samples t = nb + Rr * na of one na; a tile is T1 = 2^logT1 adjacent columns nb.  Pass 1 reads, for
// every row of its part's window of M = 2^logM rows, the T1 elements of its tile: one piece of T1 elements per (tile, row).
//   per part : Rt[part][seq][tile][na][T1]          a private window of M rows for every part
//   shared   : Rt[seq][tile][row][T1]               ONE row grid for the launch group, row 0 = first row of its first part
// Shared form: when the parts start a whole number of rows apart (rstep = part_step / Rr), part p's window is rows
// [p * rstep, p * rstep + M) of a grid common to all parts, and the M - rstep rows two neighbours share are regrouped once
// instead of twice (headline: 32 parts, M = 4096, rstep = 3252: 104908 rows instead of 131072).  The rows of a tile are padded
// to a multiple of RT_ROW_BLOCK, the rows of a k_raw_transpose block: a block never straddles two tiles, and its two-row
// 16-byte stores stay aligned for odd row counts.  Pieces shift by whole rows, so they keep their 2*T1-byte alignment.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ inline
#else
#define RT_HD inline
#endif

namespace dspsr_amd {

constexpr uint32_t RT_ROW_BLOCK = 64;      // rows per block of the regroup kernels

struct RtLayout {
  uint32_t shared;        // 1: one row grid per launch group; 0: one window per part
  uint32_t logT1;
  uint32_t rows;          // rows regrouped per (sequence, tile) and, per part form, per part
  uint32_t rows_padded;   // rows from one tile to the next
  uint64_t tile_stride, seq_stride, part_stride;   // elements
};

RT_HD RtLayout rt_layout_per_part(const int logM, const int logR, const int logT1, const uint32_t nseq)
{
  RtLayout l;
  l.shared = 0;
  l.logT1 = (uint32_t)logT1;
  l.rows = l.rows_padded = 1u << logM;
  l.tile_stride = (uint64_t)l.rows << logT1;
  l.seq_stride = (uint64_t)l.rows << logR;
  l.part_stride = l.seq_stride * nseq;
  return l;
}

// nb parts, rstep rows apart
RT_HD RtLayout rt_layout_shared(const int logM, const int logR, const int logT1, const uint32_t nb, const uint64_t rstep)
{
  RtLayout l;
  l.shared = 1;
  l.logT1 = (uint32_t)logT1;
  l.rows = (uint32_t)(rstep * (nb - 1)) + (1u << logM);
  l.rows_padded = (l.rows + RT_ROW_BLOCK - 1) & ~(RT_ROW_BLOCK - 1);
  l.tile_stride = (uint64_t)l.rows_padded << logT1;
  l.seq_stride = (uint64_t)l.rows_padded << logR;
  l.part_stride = rstep << logT1;
  return l;
}

// elements the image of nb parts of nseq sequences takes
RT_HD uint64_t rt_elems(const RtLayout& l, const int logR, const uint32_t nseq, const uint32_t nb)
{
  return l.shared ? l.seq_stride * nseq : ((uint64_t)l.rows << logR) * nseq * nb;
}

// The shared form applies when the parts lie on one row grid and overlap (rstep <= M), and its padded image is no larger than
// the per-part one (short windows: M < RT_ROW_BLOCK); y_max: the most row blocks a launch can have.
RT_HD bool rt_takes_shared(const int logM, const int logR, const uint32_t nb, const uint64_t part_step, const uint32_t y_max = 65535)
{
  if (nb < 2 || (part_step & ((1ull << logR) - 1)) != 0) return false;
  const uint64_t rstep = part_step >> logR, M = 1ull << logM;
  if (rstep == 0 || rstep > M) return false;
  const uint64_t rows = rstep * (nb - 1) + M, padded = (rows + RT_ROW_BLOCK - 1) & ~(uint64_t)(RT_ROW_BLOCK - 1);
  return padded <= M * nb && padded / RT_ROW_BLOCK <= y_max;
}

// element of column `col` of row `na` of (part, seq, tile); part counts from the launch group's first part
RT_HD uint64_t rt_offset(const RtLayout& l, const uint32_t part, const uint32_t seq, const uint32_t tile, const uint32_t na, const uint32_t col)
{
  return part * l.part_stride + seq * l.seq_stride + tile * l.tile_stride + ((uint64_t)na << l.logT1) + col;
}

}  // namespace dspsr_amd
