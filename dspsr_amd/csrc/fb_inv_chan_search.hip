// k_inv_chan with the search-mode epilogue: square-law detection + time scrunch inside the inverse pass (FB_OUT_SEARCH)
#include "fb_inv_chan.h"

namespace dspsr_amd {

template <int... I> static k3_t pick3s(int logf, bool full, bool presplit, iseq<I...>)
{
  static const k3_t t[] = {k_inv_chan<I, 2, -1>...};
  static const k3_t f[] = {k_inv_chan<I, 2, full_logt(I)>...};
  static const k3_t tp[] = {k_inv_chan<I, FB_EPI_PRESPLIT + 2, -1>...};
  static const k3_t fp[] = {k_inv_chan<I, FB_EPI_PRESPLIT + 2, full_logt(I)>...};
  return presplit ? (full ? fp[logf] : tp[logf]) : (full ? f[logf] : t[logf]);
}
k3_t fb_pick3s(int logf, bool full, bool presplit) { return pick3s(logf, full, presplit, seq_t()); }

}  // namespace dspsr_amd
