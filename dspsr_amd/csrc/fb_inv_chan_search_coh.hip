// k_inv_chan with the search-mode epilogue on the four Coherence products (digifits -p 4, digifil -d 4): detect4 + time scrunch of
// four rows per channel inside the inverse pass (FB_OUT_SEARCH with state DSPSR_AMD_COHERENCE).  A translation unit of its own: the
// square-law forms of fb_inv_chan_search.hip are compiled without these.
#include "fb_inv_chan.h"

namespace dspsr_amd {

template <int... I> static k3_t pick3c(int logf, bool full, bool presplit, iseq<I...>)
{
  static const k3_t t[] = {k_inv_chan<I, FB_EPI_COHERENCE + 2, -1>...};
  static const k3_t f[] = {k_inv_chan<I, FB_EPI_COHERENCE + 2, full_logt(I)>...};
  static const k3_t tp[] = {k_inv_chan<I, FB_EPI_COHERENCE + FB_EPI_PRESPLIT + 2, -1>...};
  static const k3_t fp[] = {k_inv_chan<I, FB_EPI_COHERENCE + FB_EPI_PRESPLIT + 2, full_logt(I)>...};
  return presplit ? (full ? fp[logf] : tp[logf]) : (full ? f[logf] : t[logf]);
}
k3_t fb_pick3c(int logf, bool full, bool presplit) { return pick3c(logf, full, presplit, seq_t()); }

}  // namespace dspsr_amd
