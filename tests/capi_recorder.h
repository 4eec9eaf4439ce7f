// Controls of the recording C-ABI (tests/capi_recorder.cpp), for tests/adaptor_trace_driver.cpp.
#pragma once
#include <stdint.h>
#include <string>

namespace rec
{
  //! a new scenario: empty log, ordinals from 0, no failure armed, scripted values at their defaults
  void reset ();
  //! a line of the driver's own in the log (printf format)
  void note (const char* fmt, ...);
  //! the next call of `function` returns `code` and leaves `message` (default: one that names the function and the code) as the
  //! context's last error
  void fail (const char* function, int code, const char* message = 0);
  //! the log of the scenario so far
  const std::string& text ();

  // ---- what the calls whose results the adaptors read return
  void set_step (uint64_t nsamp_step);                          // dspsr_amd_filterbank_sizes
  void set_fold (uint32_t hits_per_bin, uint64_t ndat_folded);  // dspsr_amd_fold_set_bins, dspsr_amd_fold_get_ndat_folded
  void set_sk_npart (uint64_t npart);                           // dspsr_amd_sk_npart
  void set_response_ndim (int ndim);                            // dspsr_amd_filterbank_response_ndim
}
