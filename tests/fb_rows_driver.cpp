// The row-overlap rule of dspsr_amd/csrc/fb_rows.h run stand-alone (tests/test_fb_rows_host.py builds this file with the address and
// undefined-behaviour sanitizers).  Cases are read from stdin until it ends, one per line:
//   nouter ninner outer_stride inner_stride row
// and answered with one line of six 0 / 1: the two predicates (outer-major, inner-major), then fb_rows_ok as the callers ask it --
// either order (perform, perform_raw, perform_detect) and outer-major only (perform_search), each for a call that writes rows and
// for one that writes none.
#include <inttypes.h>
#include <stdio.h>

#include "fb_rows.h"

using namespace dspsr_amd;

int main()
{
  uint64_t no, ni, so, si, row;
  int n;
  while ((n = scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &no, &ni, &so, &si, &row)) == 5)
    printf("%d %d %d %d %d %d\n", fb_rows_outer_major(no, ni, so, si, row) ? 1 : 0, fb_rows_inner_major(no, ni, so, si, row) ? 1 : 0,
           fb_rows_ok(1, no, ni, so, si, row, true) ? 1 : 0, fb_rows_ok(1, no, ni, so, si, row, false) ? 1 : 0,
           fb_rows_ok(0, no, ni, so, si, row, true) ? 1 : 0, fb_rows_ok(0, no, ni, so, si, row, false) ? 1 : 0);
  return n == EOF && feof(stdin) ? 0 : 2;
}
