// k_inv_chan with a matrix response (one Jones matrix per bin, Response::operate(data1, data2)): complex / detected output
#include "fb_inv_chan.h"

namespace dspsr_amd {

template <int... I> static k3_t pick3m(int logf, bool full, bool presplit, iseq<I...>)
{
  static const k3_t t[] = {k_inv_chan<I, FB_EPI_MATRIX, -1>...};
  static const k3_t f[] = {k_inv_chan<I, FB_EPI_MATRIX, full_logt(I)>...};
  static const k3_t tp[] = {k_inv_chan<I, FB_EPI_MATRIX + FB_EPI_PRESPLIT, -1>...};
  static const k3_t fp[] = {k_inv_chan<I, FB_EPI_MATRIX + FB_EPI_PRESPLIT, full_logt(I)>...};
  return presplit ? (full ? fp[logf] : tp[logf]) : (full ? f[logf] : t[logf]);
}
k3_t fb_pick3m(int logf, bool full, bool presplit) { return pick3m(logf, full, presplit, seq_t()); }

}  // namespace dspsr_amd
