// Internals of the fold engine shared with the fused filterbank+detect+fold path (not installed).
#pragma once
#include <vector>

#include "engine_internal.h"
#include "fold_plan.h"

namespace dspsr_amd {
// one run of the plan recurrence without walking its samples (host_prep.cpp)
uint64_t fold_plan_run(double* phi_io, double pps, double double_nbin, uint64_t nmax, uint32_t* ibin_out);
}  // namespace dspsr_amd

// A plan on the device.  Every consumer of the pending run-length plan (the stand-alone fold, fold_many, the fourth moments,
// the fused part plan, the four-pass segment plan) takes it through the same steps, each written once in fold.hip:
//   plan_close      the open run gets its hits; the next plan opens a fresh run
//   slot_acquire    the engine's next slot; when its last consumer is still pending, the host waits for `done` -- the pinned
//                   staging and the device copy of a slot are never rewritten before that
//   slot_reserve    the three buffer pairs, grown where the plan needs more
//   fold_plan.h     a builder fills the pinned staging
//   plan_upload     the copies, on the fold's upload stream, then `ready`
//   fold_plan_wait  the compute stream waits for `ready`, right in front of the first kernel that reads the plan
//   fold_part_plan_submitted   behind the last such kernel: `done` recorded on the compute stream, then pending = true
// Two slots, so that building and uploading the plan of block i+1 never waits for the fold kernel of block i (pinned staging
// => the H2D copies are truly asynchronous).  An empty plan, and a segment plan that does not qualify, take no slot.
struct PlanSlot {
  uint32_t* h_bin_start = nullptr;   // pinned: bin_start[nbin + 1], or the fused part plan's start[] and entries
  uint32_t* d_bin_start = nullptr;
  dspsr_amd::Interval* h_iv = nullptr;          // pinned
  dspsr_amd::Interval* d_iv = nullptr;
  uint32_t* h_aux = nullptr;         // pinned: the dense table, or the segment plan's run_off and blk_first
  uint32_t* d_aux = nullptr;
  size_t bin_cap = 0, iv_cap = 0, aux_cap = 0;
  hipEvent_t done = nullptr;         // the last consumer has read the plan
  bool pending = false;              // `done` is recorded and not yet waited for
  hipEvent_t ready = nullptr;        // the plan's copies (issued on the fold's upload stream) have landed
};

struct dspsr_amd_fold {
  dspsr_amd_ctx* ctx;
  uint32_t nchan = 0, npol = 0, ndim = 0, nbin = 0;
  float* profile = nullptr;     // [chan][pol] rows of nbin*ndim floats, `span` floats apart
  size_t profile_floats = 0;    // floats of the library-owned buffer (0 when the profile is bound to a caller's buffer)
  uint64_t span = 0;            // floats between consecutive (chan, pol) rows
  float* part = nullptr;        // partial profiles of the time segments of a long-run fold (fold.hip, FOLD_LONG_RUN)
  size_t part_floats = 0;
  bool bound = false;           // profile points into the engine-owned device PhaseSeries (dspsr_amd_fold_bind_profile)
  // run-length plan, as CUDA::FoldEngine (FoldCUDA.cu:64-113)
  hipStream_t upload = nullptr;  // plans travel host -> device beside the compute stream (see plan_upload in fold.hip)
  std::vector<dspsr_amd::RunBin> binplan;
  uint32_t current_bin = 0, current_hits = 0, folding_nbin = 0;
  uint64_t ndat_fold = 0;
  PlanSlot slot[2];
  int next_slot = 0;
  std::vector<uint32_t> cursor;
};

// The fused kernel adds a bin's samples one after the other (exact time order): a run of n samples is a dependent chain of n
// float4 adds on one thread, about 16 cycles each.  Up to this length that still costs less than the detected round trip
// through HBM (headline geometry, ms per block fused / separate: 34-sample runs 4.99 / 5.93, 136: 5.14 / 6.01, 545: 5.42 /
// 5.85, 1090: 6.39 / 5.98; tools/exp_fused_runs.py); beyond it the plan takes the separate launches and the long-run fold.
constexpr uint32_t FOLD_FUSED_MAX_RUN = 640;
// Longest run of the pending plan, open or closed (against FOLD_LONG_RUN of fold_plan.h and FOLD_FUSED_MAX_RUN)
static inline uint32_t fold_plan_max_run(const dspsr_amd_fold* f)
{
  return dspsr_amd::plan_max_run(f->binplan.data(), f->binplan.size(), f->current_hits);
}

// Fused path (filterbank.hip): the pending plan as the per-part plan of fold_plan.h on the device (*d_start, *d_iv).  The plan
// is consumed (cleared); fold_part_plan_submitted() must be called after the kernels that read it have been enqueued.
int fold_build_part_plan(dspsr_amd_fold* f, uint32_t nkeep, uint32_t npart, const uint32_t** d_start,
                         const dspsr_amd::Interval** d_iv, PlanSlot** slot);
// the compute stream waits until the plan in `slot` has landed (call right in front of the first kernel that reads it)
int fold_plan_wait(dspsr_amd_fold* f, PlanSlot* slot);
int fold_part_plan_submitted(dspsr_amd_fold* f, PlanSlot* slot);

// Four-pass fused fold (fb_four_pass.hip k_inv_b<., true>): the pending plan as the segment plan of fold_plan.h on the device.
// *ok = false: the plan does not qualify (segment_plan_qualifies) and is left pending (the caller takes Detection + Fold).
// Otherwise the plan is consumed.
int fold_build_segment_plan(dspsr_amd_fold* f, uint64_t ndat, uint32_t seg, bool* ok, const uint32_t** d_run_off,
                            const uint32_t** d_blk_first, const uint32_t** d_bin_start, const dspsr_amd::Interval** d_iv, PlanSlot** slot);
// profile[chan0 + c][bin] += the segment piece sums of the bin's intervals, in time order (c < nchan).
//   msum: [c][part][tile][t2][2] float4 (ntile = 2^logNt tiles of 2^logTt samples, Mb = 2^logMb runs per tile, run t2 of tile
//   `tile` = output positions tile*Tt + (t2 << logMa) ...); nkeep / nfilt_pos: the kept window of a part
int fold_segment_combine(dspsr_amd_fold* f, const float* msum, uint32_t chan0, uint32_t nchan, uint32_t npart, uint32_t nkeep,
                         uint32_t nfilt_pos, int logTt, int logMa, int logMb, const uint32_t* d_bin_start, const dspsr_amd::Interval* d_iv);
// profile += sum of `nseg` partial profiles (packed [seg][chan][npol][nbin][ndim]) in order: segmented fused launches, the LONG
// folds; `who` names the caller in the text of a launch error (it also reports the error of a launch just in front of it)
int fold_combine_partials(dspsr_amd_fold* f, const char* who, const float* part, uint32_t nseg, uint32_t chan0, uint32_t nchan);

// Fourth moments (fold_moments.hip).  fold_plan_to_device: the pending plan closed, bucketed by phase bin (bin_start / iv of
// *slot, as for k_fold_chunked) and uploaded; [*first, *last) its sample span with *first rounded down to a multiple of 4,
// *max_run its longest run.  The plan is consumed; fold_part_plan_submitted follows the kernels that read it.
int fold_plan_to_device(dspsr_amd_fold* f, const char* who, PlanSlot** slot, uint64_t* first, uint64_t* last, uint32_t* max_run);
// Fold::Engine::fold of a profile of npol 1 x ndim 14 from ndim 4 Stokes rows (stokes) or ndim 14 rows
int fold_moments_run(dspsr_amd_fold* f, const float* in_dev, uint64_t in_chan_stride, bool stokes, const char* who);
