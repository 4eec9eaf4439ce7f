// k_inv_chan with the fused fold of the square-law states (Intensity, PPQQ): EPI == 3
#include "fb_inv_chan.h"

namespace dspsr_amd {

template <int... I> static k3_t pick3q(int logf, bool full, bool presplit, iseq<I...>)
{
  static const k3_t t[] = {k_inv_chan<I, 3, -1>...};
  static const k3_t f[] = {k_inv_chan<I, 3, full_logt(I)>...};
  static const k3_t tp[] = {k_inv_chan<I, FB_EPI_PRESPLIT + 3, -1>...};
  static const k3_t fp[] = {k_inv_chan<I, FB_EPI_PRESPLIT + 3, full_logt(I)>...};
  return presplit ? (full ? fp[logf] : tp[logf]) : (full ? f[logf] : t[logf]);
}
k3_t fb_pick3q(int logf, bool full, bool presplit) { return pick3q(logf, full, presplit, seq_t()); }

}  // namespace dspsr_amd

FB_ST_READER(inv_chan_fold_sq)
