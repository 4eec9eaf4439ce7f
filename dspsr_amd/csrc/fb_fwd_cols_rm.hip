// Convolving filterbank, forward pass 1 with the rows of A in the mirror-paired order (fb_row_map.h): the form in front of a pass 2
// that splits the polarisations (k_fwd_rows SPLIT)
#include "fb_fwd_cols.h"

namespace dspsr_amd {

template <int... I> static k1_t pick1_rm(int logf, int raww, bool full, iseq<I...>)
{
  static const k1_t t4[] = {k_fwd_cols_rm<I, 4, -1>...};
  static const k1_t t1[] = {k_fwd_cols_rm<I, 1, -1>...};
  static const k1_t f4[] = {k_fwd_cols_rm<I, 4, full_logt(I)>...};
  static const k1_t f1[] = {k_fwd_cols_rm<I, 1, full_logt(I)>...};
  return full ? (raww == 1 ? f1[logf] : f4[logf]) : (raww == 1 ? t1[logf] : t4[logf]);
}
k1_t fb_pick1_rm(int logf, int raww, bool full) { return pick1_rm(logf, raww, full, seq_t()); }

}  // namespace dspsr_amd

FB_ST_READER(fwd_cols_rm)
