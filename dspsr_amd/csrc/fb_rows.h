// When the output rows of a filterbank call do not overlap: pure host code, standard headers only (tests/test_fb_rows_host.py runs
// it without a GPU).  nouter * ninner rows of `row` floats, row (o, i) from float o * outer_stride + i * inner_stride on; the perform
// calls take channels as the outer index and polarisations (detected: planes) as the inner one.
#pragma once
#include <stdint.h>

namespace dspsr_amd {
// outer-major (channel-major, the TimeSeries FPT order): an outer index's inner rows lie together, ahead of the next outer index's
static inline bool fb_rows_outer_major(uint64_t nouter, uint64_t ninner, uint64_t outer_stride, uint64_t inner_stride, uint64_t row)
{
  return (ninner == 1 || inner_stride >= row) && (nouter == 1 || outer_stride >= (ninner - 1) * inner_stride + row);
}
// inner-major (polarisation- or plane-major): the mirror, for more than one inner index
static inline bool fb_rows_inner_major(uint64_t nouter, uint64_t ninner, uint64_t outer_stride, uint64_t inner_stride, uint64_t row)
{
  return ninner > 1 && (nouter == 1 || outer_stride >= row) && inner_stride >= (nouter - 1) * outer_stride + row;
}
// What a perform call asks of its rows: nothing when it writes none (`written`: the parts of the call; search mode: the samples it
// completes), else one of the two orders -- the search form writes FPT rows: outer-major only
static inline bool fb_rows_ok(uint64_t written, uint64_t nouter, uint64_t ninner, uint64_t outer_stride, uint64_t inner_stride, uint64_t row,
                              bool either_order)
{
  return !written || fb_rows_outer_major(nouter, ninner, outer_stride, inner_stride, row) ||
         (either_order && fb_rows_inner_major(nouter, ninner, outer_stride, inner_stride, row));
}
}  // namespace dspsr_amd
