// Stand-alone driver of dspsr_amd/csrc/fb_rt_layout.h (tests/test_rt_layout_host.py): includes only that header and checks, for
// one geometry per input line, every offset pass 1 reads and k_raw_transpose writes.  Input line:
//   logM logR logT1 nseq nb part_step alloc_parts
// (part_step in samples; alloc_parts: the parts the image is allocated for, max_parts of the object).  Output: one line
//   shared rows rows_padded elems alloc   and one line "ok", or the first property that fails.
// With the shared form the window of part p is rows [p * rstep, p * rstep + M) of the group's row grid; a PLACE is
// (row of the grid, seq, tile) there and (part, na, seq, tile) in the per-part form.
//   * every offset of (part, seq, tile, na, col) is below the allocation and below rt_elems; the columns of a piece are adjacent
//   * distinct places have distinct, non-overlapping pieces: walked in lexicographic order their offsets grow by >= T1
//   * (p, na) and (p', na') with p * rstep + na == p' * rstep + na' have the same offset: every (p, na) lies at its row's place
//   * a piece starts at a multiple of T1 elements (2*T1 bytes of byte pairs); where k_raw_transpose stores two rows at once
//     (T1 == 4, an even row of a block of RT_ROW_BLOCK rows whose row count is even) at a multiple of 8 elements (16 bytes)
#include <stdint.h>
#include <stdio.h>

#include "fb_rt_layout.h"

using namespace dspsr_amd;

int main()
{
  long long logM, logR, logT1, nseq, nb, part_step, alloc_parts;
  while (scanf("%lld %lld %lld %lld %lld %lld %lld", &logM, &logR, &logT1, &nseq, &nb, &part_step, &alloc_parts) == 7) {
    const uint32_t M = 1u << logM, Rr = 1u << logR, T1 = 1u << logT1, ntile = Rr >> logT1;
    const bool shared = rt_takes_shared((int)logM, (int)logR, (uint32_t)nb, (uint64_t)part_step);
    const uint64_t rstep = (uint64_t)part_step >> logR;
    const RtLayout l = shared ? rt_layout_shared((int)logM, (int)logR, (int)logT1, (uint32_t)nb, rstep)
                              : rt_layout_per_part((int)logM, (int)logR, (int)logT1, (uint32_t)nseq);
    const uint64_t elems = rt_elems(l, (int)logR, (uint32_t)nseq, (uint32_t)nb);
    const uint64_t alloc = (uint64_t)alloc_parts * nseq * M * Rr;
    printf("%u %u %u %llu %llu\n", l.shared, l.rows, l.rows_padded, (unsigned long long)elems, (unsigned long long)alloc);
    const char* fail = nullptr;
    if (elems > alloc) fail = "image larger than the allocation";
    else if (l.shared != (shared ? 1u : 0u)) fail = "layout form";
    else if (shared && l.rows != rstep * (nb - 1) + M) fail = "rows";
    else if (!shared && (l.rows != M || l.rows_padded != M)) fail = "rows of the per-part form";
    else if (shared && (l.rows_padded < l.rows || l.rows_padded % RT_ROW_BLOCK != 0 || l.rows_padded - l.rows >= RT_ROW_BLOCK)) fail = "padding";
    // the place of row `row` (shared) or of (part, na) (per part), as k_raw_transpose addresses it
    auto place = [&](const uint32_t part, const uint32_t sq, const uint32_t tl, const uint64_t row) {
      return part * (shared ? 0 : l.part_stride) + sq * l.seq_stride + tl * l.tile_stride + (row << logT1);
    };
    // 1. the places in lexicographic order: pieces inside the image, aligned, not overlapping
    const uint32_t kparts = shared ? 1u : (uint32_t)nb;
    bool first = true;
    uint64_t prev = 0;
    for (uint32_t p = 0; p < kparts && !fail; p++)
      for (uint32_t sq = 0; sq < nseq && !fail; sq++)
        for (uint32_t tl = 0; tl < ntile && !fail; tl++)
          for (uint32_t row = 0; row < l.rows; row++) {
            const uint64_t o = place(p, sq, tl, row);
            if (o + T1 > elems || o + T1 > alloc) { fail = "piece beyond the image"; break; }
            if (o % T1) { fail = "piece not aligned to T1 elements"; break; }
            if (!first && o < prev + T1) { fail = "two places overlap"; break; }
            const uint32_t blk0 = row / RT_ROW_BLOCK * RT_ROW_BLOCK, blk_rows = l.rows - blk0 < RT_ROW_BLOCK ? l.rows - blk0 : RT_ROW_BLOCK;
            if (T1 == 4 && blk_rows % 2 == 0 && row % 2 == 0 && o % 8) { fail = "two-row store not 16-byte aligned"; break; }
            prev = o;
            first = false;
          }
    // 2. what pass 1 reads: every (part, na) at the place of its row
    for (uint32_t p = 0; p < nb && !fail; p++)
      for (uint32_t sq = 0; sq < nseq && !fail; sq++)
        for (uint32_t tl = 0; tl < ntile && !fail; tl++)
          for (uint32_t na = 0; na < M; na++) {
            const uint64_t o0 = rt_offset(l, p, sq, tl, na, 0);
            if (rt_offset(l, p, sq, tl, na, T1 - 1) != o0 + T1 - 1) { fail = "columns of a piece are not adjacent"; break; }
            if (o0 + T1 > elems || o0 + T1 > alloc) { fail = "offset beyond the image"; break; }
            const uint64_t want = shared ? place(0, sq, tl, p * rstep + na) : place(p, sq, tl, na);
            if (o0 != want) { fail = shared ? "a shared row has two places" : "a row is not where it was written"; break; }
          }
    puts(fail ? fail : "ok");
  }
  return 0;
}
