// Stand-alone driver of dspsr_amd/csrc/fb_row_map.h (tests/test_row_map_host.py): includes only that header and checks the
// mirror-paired row order for one (logM, logT2) per input line.  Input line:
//   logM logT2 logX3 logC
// Output: one line "ok", or the first property that fails.
//   * (block, r) -> row is a bijection of [0, M / T2) x [0, T2) onto [0, M), and rm_slot is its inverse
//   * rows 0 and M / 2 sit in block 0 (slots 0 and T2 / 2)
//   * every block holds each of its rows together with the mirror (M - row) mod M, in the slot rm_mirror names
//   * the lower half of a block is h = T2 / 2 ascending adjacent rows, the upper half walked backwards h ascending adjacent rows
//     (block 0: h - 1, and row M / 2): the runs pass 2 stores
//   * rm_xsplit_index is a bijection of [0, C) x [0, M) onto [0, C M), and the elements of X3 adjacent channels of one bin are adjacent
//   * the places rm_xrow gives the rows of either half of a block are ONE run of h places that starts at a multiple of h
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fb_row_map.h"

using namespace dspsr_amd;

int main()
{
  long long logM, logT2, logX3, logC;
  while (scanf("%lld %lld %lld %lld", &logM, &logT2, &logX3, &logC) == 4) {
    const uint32_t M = 1u << logM, T2 = 1u << logT2, h = T2 >> 1, nblock = M >> logT2;
    const char* fail = nullptr;
    std::vector<int> seen(M, 0);
    for (uint32_t b = 0; b < nblock && !fail; b++)
      for (uint32_t r = 0; r < T2; r++) {
        const uint32_t row = rm_row((int)logM, (int)logT2, b, r);
        if (row >= M) { fail = "row out of range"; break; }
        if (seen[row]++) { fail = "two slots hold one row"; break; }
        const RowSlot s = rm_slot((int)logM, (int)logT2, row);
        if (s.block != b || s.r != r) { fail = "rm_slot is not the inverse of rm_row"; break; }
        const uint32_t rm = rm_mirror((int)logT2, b, r);
        if (rm >= T2) { fail = "mirror slot out of range"; break; }
        if (rm_row((int)logM, (int)logT2, b, rm) != ((M - row) & (M - 1))) { fail = "the mirror slot does not hold row M - m"; break; }
        if (rm_mirror((int)logT2, b, rm) != r) { fail = "the mirror of the mirror is another slot"; break; }
        // runs: lower half ascending, upper half descending (block 0: slot h is row M / 2)
        if (r < h && row != b * h + r) { fail = "lower half not ascending from h * block"; break; }
        if (r > h && row + 1 != rm_row((int)logM, (int)logT2, b, r - 1) && !(b == 0 && r == h + 1)) { fail = "upper half not descending"; break; }
      }
    for (uint32_t row = 0; row < M && !fail; row++)
      if (seen[row] != 1) fail = "a row has no slot";
    for (uint32_t b = 0; b < nblock && !fail; b++)
      for (uint32_t half = 0; half < 2 && !fail; half++) {
        uint32_t lo = M, hi = 0;
        for (uint32_t q = 0; q < h; q++) {
          const uint32_t p = rm_xrow((int)logM, rm_row((int)logM, (int)logT2, b, half * h + q));
          if (p >= M) { fail = "place out of range"; break; }
          lo = p < lo ? p : lo;
          hi = p > hi ? p : hi;
        }
        if (!fail && (hi - lo != h - 1 || lo % h != 0)) fail = "the places of a half block are not one aligned run";
      }
    if (!fail) {
      const RowSlot s0 = rm_slot((int)logM, (int)logT2, 0), sh = rm_slot((int)logM, (int)logT2, M >> 1);
      if (s0.block != 0 || s0.r != 0 || sh.block != 0 || sh.r != h) fail = "rows 0 and M / 2 are not in block 0, slots 0 and T2 / 2";
    }
    if (!fail) {
      const uint32_t C = 1u << logC, X3 = 1u << logX3;
      std::vector<unsigned char> hit((size_t)C * M, 0);
      for (uint32_t c = 0; c < C && !fail; c++)
        for (uint32_t m = 0; m < M; m++) {
          const uint64_t i = rm_xsplit_index((int)logM, (int)logX3, c, m);
          if (i >= (uint64_t)C * M) { fail = "X' index beyond the spectrum"; break; }
          if (hit[i]++) { fail = "two elements at one X' index"; break; }
          if ((c & (X3 - 1)) && i != rm_xsplit_index((int)logM, (int)logX3, c - 1, m) + 1) { fail = "channels of a layout block not adjacent"; break; }
        }
    }
    printf("%s\n", fail ? fail : "ok");
  }
  return 0;
}
