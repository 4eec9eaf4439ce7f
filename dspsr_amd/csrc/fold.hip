// dsp::Fold::Engine for gfx950 (Signal/Pulsar/dsp/Fold.h:249-312).
// Reference: host plan loop Fold.C:744-787, CPU accumulate Fold.C:835-891, CUDA twin FoldCUDA.cu
// (set_bin run-length builder :84-113, send_binplan :154-198, fold1bin* kernels :208-576).
//
// Differences by design (DESIGN.md "Fold"): the reference GPU kernels sum each run-length
// interval from zero and atomicAdd it into the profile (order-dependent float sums).  Here
// every (chan, pol, bin) accumulator is owned by exactly one thread that walks the bin's
// intervals in time order and adds sample by sample, i.e. the SAME association order as the
// CPU loop Fold.C:844-852 -- results are deterministic and bit-identical to the CPU fold of
// the same detected samples.
#include <algorithm>
#include <string.h>
#include <math.h>
#include <vector>

#include "engine_internal.h"
#include "fold_internal.h"
#include "fold_walk.h"

namespace dspsr_amd {


// Direct variant: every bin-owner thread reads its samples straight from global memory
// (used when nbin is too large for the chunked kernel).
template <int NDIM>
__global__ void k_fold_direct(const float* __restrict__ in, const uint64_t chan_stride, const uint64_t pol_stride,
                              float* __restrict__ prof, const uint64_t prof_span, const uint32_t nbin,
                              const uint32_t* __restrict__ bin_start, const Interval* __restrict__ iv)
{
  const uint32_t ipol = blockIdx.x, npol = gridDim.x, ichan = blockIdx.y;
  const float* __restrict__ row = in + ichan * chan_stride + ipol * pol_stride;
  float* __restrict__ out = prof + ((uint64_t)ichan * npol + ipol) * prof_span;
  for (uint32_t b = blockIdx.z + gridDim.z * threadIdx.x; b < nbin; b += gridDim.z * blockDim.x) {
    const uint32_t i0 = bin_start[b], i1 = bin_start[b + 1];
    if (i0 == i1) continue;
    float acc[NDIM];
#pragma unroll
    for (int d = 0; d < NDIM; d++) acc[d] = out[b * NDIM + d];
    for (uint32_t i = i0; i < i1; i++) {
      const Interval v = iv[i];
      const float* __restrict__ x = row + v.offset * NDIM;
      for (uint32_t h = 0; h < v.hits; h++)
#pragma unroll
        for (int d = 0; d < NDIM; d++) acc[d] += x[h * NDIM + d];
    }
#pragma unroll
    for (int d = 0; d < NDIM; d++) out[b * NDIM + d] = acc[d];
  }
}

// Chunked variant (the hot one).  One workgroup per (channel, pol) row.  The row is streamed
// through LDS in chunks of FOLD_CHUNK samples with fully coalesced 16-byte loads (the next
// chunk is already in flight in registers while the current one is folded); thread b owns phase
// bins b, b+blockDim, ... and walks each bin's time-ordered interval list with a cursor, adding
// the samples that fall inside the current chunk one by one.  Per (chan, pol, bin, dim) the adds
// therefore happen in time order, as in Fold.C:844-852.  With few (chan, pol) rows the bins of a row are dealt to
// gridDim.z workgroups (each streams the whole row: the re-reads come from L2 / Infinity Cache), so that the chip
// is filled without touching the order of any sum.
// (FOLD_CHUNK samples per chunk, FOLD_BPT bins per thread: fold_plan.h, with the host's tables and launch shapes; the chunk
//  stream, the cursor and the adds: fold_walk.h, shared by all kernels below and k_fold_moments)
// LONG runs.  A sum in strict time order is one dependent chain of float adds per (chan, pol, bin, dim): with phase bins
// hundreds of samples wide only a couple of chains are alive per row and the kernel is bound by the add latency (10 ms per
// 4 M samples and row at -F 64:D, profiles/r02j).  When the plan holds a run of FOLD_LONG_RUN samples or more, the host
// picks the LONG variant for the whole call: every chunk is first reduced, by all threads, to the sums of its aligned
// FOLD_MB-sample micro-blocks (each summed in time order); a bin's owner then adds, in time order, single samples up to
// the first micro-block boundary inside its run, whole micro-block sums, and single samples after the last boundary.
// Deterministic, no longer the association of the CPU loop: it agrees with it to float rounding, like the reference's own
// GPU fold (FoldCUDA.cu:208-269 sums each run from zero and adds the run sums atomically).  The association depends on the
// plan, the chunk grid and the number of time segments, each summed from zero and added to the profile in segment order by
// k_fold_combine; the segment count follows from the device's compute units and nchan*npol (fold_plan.h fold_shape), so the
// sums are reproducible on one device and row count, not across them.  Plans of shorter runs keep the exact time-order kernel.

// NROW: polarisation rows of one channel folded by the same workgroup (detected data with ndim < 4 lie in 4/ndim planes:
// the walk through the bin plan -- most of the work with 4-byte samples -- then serves all planes; the sums of every
// (chan, pol, bin, dim) keep their order).
template <int NDIM, bool LONG, int NROW>
__global__ __launch_bounds__(1024) void k_fold_chunked(const float* __restrict__ in, const uint64_t chan_stride,
                                                       const uint64_t pol_stride, float* __restrict__ prof,
                                                       const uint64_t prof_span, const uint32_t nbin,
                                                       const uint32_t* __restrict__ bin_start,
                                                       const Interval* __restrict__ iv, const uint64_t first,
                                                       const uint64_t last /* [first,last): sample span of the plan */,
                                                       float* __restrict__ part /* LONG: [seg][row][nbin][NDIM] partial sums */,
                                                       const uint32_t chunks_per_seg /* LONG: chunks per blockIdx.z */)
{
  extern __shared__ __attribute__((aligned(16))) float fold_lds[];   // NROW x FOLD_CHUNK * NDIM floats (+ micro-block sums, LONG)
  typedef FoldImage<NDIM> Img;
  constexpr uint32_t RS = Img::RS, MS = Img::MS;
  const uint32_t ipol = blockIdx.x * NROW, npol = gridDim.x * NROW, ichan = blockIdx.y;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const float* __restrict__ row = in + ichan * chan_stride + ipol * pol_stride;          // row r: + r * pol_stride
  // LONG: blockIdx.z is a TIME segment of the row (all bins), summed from zero into this segment's partial profile --
  // every sample of the row is read once; k_fold_combine adds the partials to the profile in time order.
  // exact: blockIdx.z deals the BINS of a row to gridDim.z workgroups, each streams the whole row and owns its sums.
  float* __restrict__ out = LONG ? part + (((uint64_t)blockIdx.z * gridDim.y + ichan) * npol + ipol) * nbin * NDIM
                                 : prof + ((uint64_t)ichan * npol + ipol) * prof_span;
  const uint64_t out_rs = LONG ? (uint64_t)nbin * NDIM : prof_span;                        // row r: + r * out_rs
  const uint32_t bz = LONG ? 0u : blockIdx.z, nz = LONG ? 1u : gridDim.z;

  FoldCursor cu[FOLD_BPT];
  float acc[FOLD_BPT][NROW][NDIM];
  bool touched[FOLD_BPT];
#pragma unroll
  for (int j = 0; j < FOLD_BPT; j++) {
    const uint32_t b = bz + nz * (tid + j * nt);   // bins are dealt to the nz workgroups of a row
    cu[j].open<LONG>(bin_start, iv, b, b < nbin, first + (uint64_t)blockIdx.z * chunks_per_seg * FOLD_CHUNK);
    touched[j] = LONG ? (b < nbin) : !cu[j].empty();
#pragma unroll
    for (int r = 0; r < NROW; r++)
#pragma unroll
      for (int d = 0; d < NDIM; d++) acc[j][r][d] = (!LONG && b < nbin && touched[j]) ? out[r * out_rs + b * NDIM + d] : 0.f;
  }

  // chunk c covers samples [first + c*FOLD_CHUNK, ...); rows are 16-byte aligned when first*NDIM % 4 == 0,
  // the host guarantees it by rounding `first` down
  const float* __restrict__ src0 = row + first * NDIM;
  const uint64_t nfl_total = (last - first) * NDIM;      // floats in the span
  const uint32_t nchunk_all = (uint32_t)((last - first + FOLD_CHUNK - 1) / FOLD_CHUNK);
  const uint32_t cbeg = LONG ? blockIdx.z * chunks_per_seg : 0u;
  const uint32_t nchunk = LONG ? (cbeg + chunks_per_seg < nchunk_all ? cbeg + chunks_per_seg : nchunk_all) : nchunk_all;
  float4 pre[NROW][Img::MAXR];
  if (cbeg < nchunk) fold_fetch<Img::NF4>(pre, src0, pol_stride, nfl_total, cbeg, tid, nt);
  for (uint32_t c = cbeg; c < nchunk; c++) {
    __syncthreads();                                    // previous chunk fully consumed
    fold_store<Img::NF4>(fold_lds, pre, tid, nt);
    if (c + 1 < nchunk) fold_fetch<Img::NF4>(pre, src0, pol_stride, nfl_total, c + 1, tid, nt);
    __syncthreads();
    if constexpr (LONG) {                                 // level 1: sums of the aligned micro-blocks of this chunk
      float* mbs = fold_lds + NROW * RS;
      for (uint32_t q = tid; q < NROW * MS; q += nt) {
        const uint32_t rw = q / MS, qr = q - rw * MS, mb = qr / NDIM, d = qr % NDIM;
        float sacc = 0.f;
#pragma unroll 8
        for (uint32_t h = 0; h < FOLD_MB; h++) sacc += fold_lds[rw * RS + (mb * FOLD_MB + h) * NDIM + d];
        mbs[q] = sacc;
      }
      __syncthreads();
    }
    const uint64_t c0 = first + (uint64_t)c * FOLD_CHUNK, c1 = c0 + FOLD_CHUNK;
#pragma unroll
    for (int j = 0; j < FOLD_BPT; j++) {
      while (cu[j].before(c1)) {
        uint32_t s0, n;
        cu[j].clip(c0, c1, s0, n);
        if constexpr (LONG)
          fold_long_piece(s0, s0 + n, [&](const uint32_t h0, const uint32_t h1) { fold_run_add<RS>(acc[j], fold_lds, h0, h1 - h0); },
                          [&](const uint32_t m0, const uint32_t m1) { fold_run_add<MS>(acc[j], fold_lds + NROW * RS, m0, m1 - m0); });
        else
          fold_run_add<RS>(acc[j], fold_lds, s0, n);
        if (!cu[j].advance(iv, c1)) break;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < FOLD_BPT; j++) {
    const uint32_t b = bz + nz * (tid + j * nt);
    if (b < nbin && touched[j]) fold_acc_store(acc[j], out, out_rs, b * NDIM);
  }
}


// Dense variant (round 4).  The walk above takes its intervals from global memory; the loads are small, but the per-wave
// vector-memory counter is in order, so every `s_waitcnt` in front of an interval's use also waits for the NEXT chunk's
// prefetch, issued just before -- a workgroup has bytes in flight for part of its time only (0.50 of the HBM peak on the
// reference's fold benchmark).  When no phase bin receives more than ONE run of samples per chunk (always, once the folding
// period exceeds FOLD_CHUNK samples: Benchmark/fold.csh 2794, the headline's detected series 34816) the plan is a dense table
//   tab[chunk][bin] = first sample of the run inside the chunk | samples << 11      (0: none; runs are cut at chunk ends)
// built on the host from the same run-length plan.  A thread's entries for chunk c + 1 travel with the prefetch of chunk c + 1
// and are waited for together with it at the top of the next iteration: the add phase issues no vector-memory instruction and
// no wait, so the prefetch stays in flight across it.  Same bins per thread, same chunk grid, one run per (chunk, bin) in
// chunk order: every (chan, pol, bin, dim) sum has exactly the association of k_fold_chunked<., false, .> and of Fold.C:844-852.
template <int NDIM, int NROW>
__global__ __launch_bounds__(1024) void k_fold_dense(const float* __restrict__ in, const uint64_t chan_stride,
                                                     const uint64_t pol_stride, float* __restrict__ prof,
                                                     const uint64_t prof_span, const uint32_t nbin,
                                                     const uint32_t* __restrict__ tab, const uint64_t first, const uint64_t last)
{
  extern __shared__ __attribute__((aligned(16))) float fold_lds[];   // NROW x FOLD_CHUNK * NDIM floats
  typedef FoldImage<NDIM> Img;
  const uint32_t ipol = blockIdx.x * NROW, npol = gridDim.x * NROW, ichan = blockIdx.y;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const float* __restrict__ row = in + ichan * chan_stride + ipol * pol_stride;
  float* __restrict__ out = prof + ((uint64_t)ichan * npol + ipol) * prof_span;
  const uint32_t bz = blockIdx.z, nz = gridDim.z;
  uint32_t bin[FOLD_BPT];
  float acc[FOLD_BPT][NROW][NDIM];
#pragma unroll
  for (int j = 0; j < FOLD_BPT; j++) {
    bin[j] = bz + nz * (tid + j * nt);
#pragma unroll
    for (int r = 0; r < NROW; r++)
#pragma unroll
      for (int d = 0; d < NDIM; d++) acc[j][r][d] = bin[j] < nbin ? out[r * prof_span + bin[j] * NDIM + d] : 0.f;
  }
  const float* __restrict__ src0 = row + first * NDIM;
  const uint64_t nfl_total = (last - first) * NDIM;
  const uint32_t nchunk = (uint32_t)((last - first + FOLD_CHUNK - 1) / FOLD_CHUNK);
  float4 pre[NROW][Img::MAXR];
  uint32_t tabn[FOLD_BPT];
  auto fetch = [&](const uint32_t c) {                    // a chunk and, travelling with it, the thread's table entries for it
    fold_fetch<Img::NF4>(pre, src0, pol_stride, nfl_total, c, tid, nt);
    const uint32_t* __restrict__ tc = tab + (uint64_t)c * nbin;
#pragma unroll
    for (int j = 0; j < FOLD_BPT; j++) tabn[j] = bin[j] < nbin ? tc[bin[j]] : 0u;
  };
  if (nchunk) fetch(0);
  for (uint32_t c = 0; c < nchunk; c++) {
    __syncthreads();                                    // previous chunk fully consumed
    fold_store<Img::NF4>(fold_lds, pre, tid, nt);
    uint32_t tabc[FOLD_BPT];
#pragma unroll
    for (int j = 0; j < FOLD_BPT; j++) tabc[j] = tabn[j];
    if (c + 1 < nchunk) fetch(c + 1);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FOLD_BPT; j++) fold_dense_add<Img::RS>(acc[j], fold_lds, tabc[j]);
  }
#pragma unroll
  for (int j = 0; j < FOLD_BPT; j++)
    if (bin[j] < nbin) fold_acc_store(acc[j], out, prof_span, bin[j] * NDIM);
}

// Several plans over the SAME detected rows (dspsr_amd_fold_fold_many: one Fold per pulsar, LoadToFold1.C:939-960).  Each
// chunk of the rows is read from HBM into LDS once and folded into every plan of the group while it sits there.  The
// (plan, bin) pairs of the group are laid end to end as "slots" -- plan k owns slots [slot0, slot0 + nbin) -- and the slots
// are dealt to threads exactly as k_fold_chunked deals the bins of one plan: thread t of workgroup bz owns slots
// bz + nz * (t + j * blockDim), j < FOLD_BPT, so a group of P plans costs the registers of ONE plan's walk (no per-plan
// accumulator arrays, no scratch).  Per slot the plan is either dense (a per-chunk table as k_fold_dense, built over the
// group's chunk grid, its entries travelling with the chunk prefetch) or a walk (the time-ordered interval list of
// k_fold_chunked<., false, .>).  Either way one thread owns the (chan, pol, bin, dim) sum, starts it from the profile and adds
// the samples one by one in time order: every profile is bit-identical to dspsr_amd_fold_fold of that plan alone.  The
// chunk grid starts at the group's first sample; plans with later spans simply meet their first interval later.
constexpr uint32_t FOLD_MANY_MAX = DSPSR_AMD_FOLD_MANY_MAX;   // plans per launch (bigger sets are split into several launches)
struct FoldManyPlan {
  float* prof;                  // profile, rows `span` floats apart
  uint64_t span;
  const uint32_t* bin_start;    // walk: intervals of bin b are iv[bin_start[b] .. bin_start[b+1])
  const Interval* iv;
  const uint32_t* tab;          // dense: tab[chunk * nbin + bin] over the group's chunk grid; NULL: walk
  uint32_t nbin, slot0;
};
struct FoldManyArgs { FoldManyPlan p[FOLD_MANY_MAX]; uint32_t nplan, nslot; };
// (pointers read from LDS are generic: cast to the global address space, or the loads become flat loads whose waits also drain
//  LDS traffic)
typedef __attribute__((address_space(1))) const Interval* GlobalIv;
typedef __attribute__((address_space(1))) const uint32_t* GlobalU32;

// (FOLD_MANY_THREADS = 512 threads at most, fold_plan.h: with FOLD_BPT slots of cursor, table entry and accumulators per thread
//  the 128 VGPRs of a 1024-thread workgroup spill; a group of many bins takes more workgroups per row instead)
template <int NDIM, int NROW>
__global__ __launch_bounds__(FOLD_MANY_THREADS) void k_fold_many(const float* __restrict__ in, const uint64_t chan_stride,
                                                    const uint64_t pol_stride, const FoldManyArgs a, const uint64_t first,
                                                    const uint64_t last)
{
  extern __shared__ __attribute__((aligned(16))) float fold_lds[];   // NROW x FOLD_CHUNK * NDIM floats
  // the plan descriptors, copied once from the kernel arguments with constant indices (a divergent index into the
  // argument struct could make the compiler copy it to scratch); a slot's plan is then an LDS read away
  __shared__ FoldManyPlan desc[FOLD_MANY_MAX];
  typedef FoldImage<NDIM> Img;
  const uint32_t bz = blockIdx.x, nz = gridDim.x;
  const uint32_t ipol = blockIdx.y * NROW, npol = gridDim.y * NROW, ichan = blockIdx.z;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const float* __restrict__ row = in + ichan * chan_stride + ipol * pol_stride;
  if (tid == 0) {
#pragma unroll
    for (uint32_t k = 0; k < FOLD_MANY_MAX; k++) desc[k] = a.p[k];
  }
  __syncthreads();
  // per owned slot: plan k and bin b (k = FOLD_MANY_MAX: no slot), the walk cursor, the dense table entry
  uint32_t pk[FOLD_BPT], bin[FOLD_BPT], tabn[FOLD_BPT];
  FoldCursor cu[FOLD_BPT];
  float acc[FOLD_BPT][NROW][NDIM];
  bool touched[FOLD_BPT];
#pragma unroll
  for (int j = 0; j < FOLD_BPT; j++) {
    const uint32_t s = bz + nz * (tid + j * nt);
    uint32_t k = FOLD_MANY_MAX;
#pragma unroll
    for (uint32_t q = 0; q < FOLD_MANY_MAX; q++)
      if (q < a.nplan && s >= a.p[q].slot0 && s < a.nslot) k = q;      // (slot0 ascending)
    pk[j] = k;
    bin[j] = k < FOLD_MANY_MAX ? s - desc[k].slot0 : 0u;
    tabn[j] = 0;
    const bool dense = k < FOLD_MANY_MAX && desc[k].tab;
    const uint32_t kk = k < FOLD_MANY_MAX ? k : 0u;
    cu[j].open<false>((GlobalU32)desc[kk].bin_start, (GlobalIv)desc[kk].iv, bin[j], k < FOLD_MANY_MAX && !dense, 0);
    touched[j] = dense || !cu[j].empty();
    const float* __restrict__ out = touched[j] ? desc[k].prof + ((uint64_t)ichan * npol + ipol) * desc[k].span : nullptr;
#pragma unroll
    for (int r = 0; r < NROW; r++)
#pragma unroll
      for (int d = 0; d < NDIM; d++) acc[j][r][d] = touched[j] ? out[r * desc[k].span + bin[j] * NDIM + d] : 0.f;
  }
  const float* __restrict__ src0 = row + first * NDIM;
  const uint64_t nfl_total = (last - first) * NDIM;
  const uint32_t nchunk = (uint32_t)((last - first + FOLD_CHUNK - 1) / FOLD_CHUNK);
  float4 pre[NROW][Img::MAXR];
  auto fetch = [&](const uint32_t c) {                    // a chunk and, travelling with it, the dense slots' table entries for it
    fold_fetch<Img::NF4>(pre, src0, pol_stride, nfl_total, c, tid, nt);
#pragma unroll
    for (int j = 0; j < FOLD_BPT; j++) {
      const bool dense = pk[j] < FOLD_MANY_MAX && desc[pk[j]].tab;
      tabn[j] = dense ? ((GlobalU32)desc[pk[j]].tab)[(uint64_t)c * desc[pk[j]].nbin + bin[j]] : 0u;
    }
  };
  if (nchunk) fetch(0);
  for (uint32_t c = 0; c < nchunk; c++) {
    __syncthreads();                                    // previous chunk fully consumed
    // (fold_walk.h's fold_store, written out: called as a function here, k_fold_many<4, 1> copies one prefetched float4 right behind
    //  its load, and the s_waitcnt vmcnt(0) in front of the copy drains the whole prefetch in every chunk: 7 % at 128 channels x 2^20
    //  samples, profiles/HISTORY.md)
#pragma unroll
    for (int rw = 0; rw < NROW; rw++)
#pragma unroll
      for (uint32_t r = 0; r < Img::MAXR; r++)
        if (tid + r * nt < Img::NF4) ((float4*)(fold_lds + rw * Img::RS))[tid + r * nt] = pre[rw][r];
    uint32_t tabc[FOLD_BPT];
#pragma unroll
    for (int j = 0; j < FOLD_BPT; j++) tabc[j] = tabn[j];
    if (c + 1 < nchunk) fetch(c + 1);
    __syncthreads();
    const uint64_t c0 = first + (uint64_t)c * FOLD_CHUNK, c1 = c0 + FOLD_CHUNK;
#pragma unroll
    for (int j = 0; j < FOLD_BPT; j++) {
      fold_dense_add<Img::RS>(acc[j], fold_lds, tabc[j]);  // dense slot: at most one run in this chunk (walk slot: entry 0, nothing)
      while (cu[j].before(c1)) {              // walk slot
        uint32_t s0, n;
        cu[j].clip(c0, c1, s0, n);
        fold_run_add<Img::RS>(acc[j], fold_lds, s0, n);
        if (!cu[j].advance((GlobalIv)desc[pk[j]].iv, c1)) break;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < FOLD_BPT; j++) {
    if (!touched[j]) continue;
    const uint32_t k = pk[j];
    fold_acc_store(acc[j], desc[k].prof + ((uint64_t)ichan * npol + ipol) * desc[k].span, desc[k].span, bin[j] * NDIM);
  }
}

// LONG: profile[row][bin][dim] += partial sums of the time segments, in time order
__global__ __launch_bounds__(256) void k_fold_combine(float* __restrict__ prof, const uint64_t prof_span, const float* __restrict__ part,
                                                      const uint32_t nrow, const uint32_t row_floats, const uint32_t nseg)
{
  const uint64_t n = (uint64_t)nrow * row_floats;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = i / row_floats, k = i - r * row_floats;
    float a = prof[r * prof_span + k];
    for (uint32_t sg = 0; sg < nseg; sg++) a += part[(uint64_t)sg * n + i];
    prof[r * prof_span + k] = a;
  }
}

// Zeroed samples (Fold.C:853-866, FoldCUDA.cu:415-470 fold1bin*hits): when the input carries zeroed (RFI-excised) samples
// the number of samples a bin really received differs from channel to channel, so hits[] is kept per channel and counts,
// for polarisation 0, the samples whose first float is not zero.  One thread per (channel, bin) walks the bin's intervals.
__global__ __launch_bounds__(256) void k_fold_count_hits(const float* __restrict__ in, const uint64_t chan_stride, const uint32_t ndim,
                                                         uint32_t* __restrict__ hits, const uint32_t nbin,
                                                         const uint32_t* __restrict__ bin_start, const Interval* __restrict__ iv)
{
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (b >= nbin) return;
  const float* __restrict__ row = in + c * chan_stride;
  uint32_t n = 0;
  for (uint32_t i = bin_start[b]; i < bin_start[b + 1]; i++) {
    const Interval v = iv[i];
    const float* __restrict__ x = row + v.offset * ndim;
    for (uint32_t h = 0; h < v.hits; h++) n += x[(uint64_t)h * ndim] != 0.0f;
  }
  hits[(uint64_t)c * nbin + b] += n;
}

// Four-pass fused fold, second half: thread (chan, bin) walks the bin's intervals in time order and adds the piece sums
// k_inv_b<., true> left for every Tt-sample segment the interval covers: piece A of a segment entered at its first kept
// sample, piece B of a segment entered behind its cut (fold_internal.h).  One dependent chain of float4 adds per
// (chan, bin), 1/Tt of the samples long.
__global__ __launch_bounds__(256) void k_fold_segsum(float* __restrict__ prof, const uint64_t prof_span, const uint32_t nbin,
                                                     const float4* __restrict__ msum, const uint32_t npart, const uint32_t nkeep,
                                                     const uint32_t nfilt_pos, const int logTt, const int logMa, const int logMb,
                                                     const uint32_t* __restrict__ bin_start, const Interval* __restrict__ iv)
{
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (b >= nbin) return;
  const uint32_t i0 = bin_start[b], i1 = bin_start[b + 1];
  if (i0 == i1) return;
  const int logNt = logMa - logTt;                        // tiles (blocks of Tt values of t1) per channel
  const uint32_t hi = nfilt_pos + nkeep;
  float4* __restrict__ pp = (float4*)(prof + (uint64_t)c * prof_span) + b;
  float4 acc = *pp;
  const float4* __restrict__ mc = msum + (((uint64_t)c * npart) << (logNt + logMb + 1));
  // The pieces are fetched eight at a time and added in time order: their addresses depend on the plan alone (one load per
  // iteration, with a 64-bit division in front of it, left this kernel at one memory round trip per segment: 180 us per block
  // at -F 64:D).  `next` steps through the segments of the bin's intervals; part and position advance without divisions.
  uint32_t i = i0;
  uint64_t idat = 0, end = 0;
  uint32_t part = 0, pos = 0;
  auto next = [&](uint64_t& a) -> bool {
    while (idat >= end) {
      if (i >= i1) return false;
      const Interval v = iv[i++];
      idat = v.offset;
      end = v.offset + v.hits;
      part = (uint32_t)(idat / nkeep);
      pos = (uint32_t)(idat - (uint64_t)part * nkeep) + nfilt_pos;
    }
    const uint32_t seg = pos >> logTt;                                          // position = seg*Tt + j = t1 + (t2 << logMa)
    const uint32_t first = (seg << logTt) > nfilt_pos ? (seg << logTt) : nfilt_pos;         // the segment's first kept position
    const uint32_t last = ((seg + 1) << logTt) < hi ? ((seg + 1) << logTt) : hi;           // one past its last kept position
    const uint32_t t1blk = seg & ((1u << logNt) - 1), t2 = seg >> logNt;
    a = (((((uint64_t)part << logNt) + t1blk) << logMb) + t2) * 2 + (pos == first ? 0 : 1);
    idat += last - pos;                                // to the segment's end (an interval that ends inside took piece A, which ends there)
    pos = last;
    if (pos >= hi) { part++; pos = nfilt_pos; }        // the interval goes on in the next part
    return true;
  };
  for (;;) {
    float4 q[8];
    int n = 0;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      uint64_t a;
      if (n == u && next(a)) { q[u] = mc[a]; n = u + 1; }
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (u < n) { acc.x += q[u].x; acc.y += q[u].y; acc.z += q[u].z; acc.w += q[u].w; }
    if (n < 8) break;
  }
  *pp = acc;
}

}  // namespace dspsr_amd

using namespace dspsr_amd;

static void slot_free(PlanSlot& s)
{
  if (s.h_bin_start) (void)hipHostFree(s.h_bin_start);
  if (s.h_iv) (void)hipHostFree(s.h_iv);
  if (s.d_bin_start) (void)hipFree(s.d_bin_start);
  if (s.d_iv) (void)hipFree(s.d_iv);
  if (s.h_aux) (void)hipHostFree(s.h_aux);
  if (s.d_aux) (void)hipFree(s.d_aux);
  if (s.done) (void)hipEventDestroy(s.done);
  if (s.ready) (void)hipEventDestroy(s.ready);
  s = PlanSlot();
}

// one pinned / device buffer pair of a slot: at least `need` elements, `alloc` of them when it has to grow
template <class T>
static bool slot_grow(T*& h, T*& d, size_t& cap, size_t need, size_t alloc)
{
  if (need <= cap) return true;
  if (h) (void)hipHostFree(h);
  if (d) (void)hipFree(d);
  h = nullptr; d = nullptr; cap = 0;
  if (hipHostMalloc((void**)&h, alloc * sizeof(T)) != hipSuccess) return false;
  if (hipMalloc((void**)&d, alloc * sizeof(T)) != hipSuccess) return false;
  cap = alloc;
  return true;
}

// the words are sized exactly (nbin + 1 hardly ever changes); intervals and aux words follow the plan and grow with headroom
static bool slot_reserve(PlanSlot& s, size_t nwords, size_t niv, size_t naux)
{
  if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) return false;
  if (!s.ready && hipEventCreateWithFlags(&s.ready, hipEventDisableTiming) != hipSuccess) return false;
  return slot_grow(s.h_bin_start, s.d_bin_start, s.bin_cap, nwords, nwords) &&
         slot_grow(s.h_iv, s.d_iv, s.iv_cap, niv, niv + niv / 2 + 16) &&
         slot_grow(s.h_aux, s.d_aux, s.aux_cap, naux, naux + naux / 4 + 1024);
}

// FoldCUDA.cu:163-164: the open run gets its hits.  The plan is used up: the next one opens a fresh run (as after set_nbin).
static void plan_close(dspsr_amd_fold* f)
{
  if (f->current_hits && !f->binplan.empty()) f->binplan.back().hits = f->current_hits;
  f->current_hits = 0;
  f->current_bin = f->folding_nbin;
}

// The engine's next slot.  The fold that last used it (two plans ago) must have consumed it before the host rewrites it.
static int slot_acquire(dspsr_amd_fold* f, const char* who, PlanSlot** out)
{
  PlanSlot& sl = f->slot[f->next_slot];
  f->next_slot ^= 1;
  if (sl.pending) {
    const hipError_t e = hipEventSynchronize(sl.done);
    if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(e));
    sl.pending = false;
  }
  *out = &sl;
  return DSPSR_AMD_OK;
}

// Plans go to the device on the fold's own stream, not in the compute stream: there a pair of small host-to-device copies
// stood between the last kernel of one block and the first of the next (about 45 us of idle device per block in the kernel
// trace, 3.5 % of a cfg4 block), although the kernel that reads the plan is launched several passes later.  The pinned
// source and the device copy of a slot are only rewritten after its `done` event (recorded on the compute stream behind the
// consumer) has been waited for on the host.
struct PlanCopy { void* dst; const void* src; size_t bytes; };
static hipError_t plan_upload(dspsr_amd_fold* f, PlanSlot& sl, const PlanCopy* c, const int n)
{
  hipError_t e = hipSuccess;
  if (!f->upload) e = hipStreamCreateWithFlags(&f->upload, hipStreamNonBlocking);
  for (int i = 0; i < n && e == hipSuccess; i++)
    if (c[i].bytes) e = hipMemcpyAsync(c[i].dst, c[i].src, c[i].bytes, hipMemcpyHostToDevice, f->upload);
  if (e == hipSuccess) e = hipEventRecord(sl.ready, f->upload);
  return e;
}
int fold_plan_wait(dspsr_amd_fold* f, PlanSlot* slot)
{
  const hipError_t e = hipStreamWaitEvent(f->ctx->stream, slot->ready, 0);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "fold: plan wait: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
// behind the last kernel that reads the plan: pending only once `done` is recorded
static int slot_submit(dspsr_amd_fold* f, const char* who, PlanSlot& sl)
{
  const hipError_t e = hipEventRecord(sl.done, f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(e));
  sl.pending = true;
  return DSPSR_AMD_OK;
}
int fold_part_plan_submitted(dspsr_amd_fold* f, PlanSlot* slot) { return slot_submit(f, "fused fold", *slot); }

extern "C" int dspsr_amd_fold_create(dspsr_amd_ctx* ctx, dspsr_amd_fold** out)
{
  if (!ctx || !out) return DSPSR_AMD_EINVAL;
  dspsr_amd_fold* f = new dspsr_amd_fold;
  f->ctx = ctx;
  *out = f;
  return DSPSR_AMD_OK;
}

extern "C" void dspsr_amd_fold_destroy(dspsr_amd_fold* f)
{
  if (!f) return;
  (void)hipStreamSynchronize(f->ctx->stream);
  if (f->profile && !f->bound) (void)hipFree(f->profile);
  if (f->part) (void)hipFree(f->part);
  if (f->upload) { (void)hipStreamSynchronize(f->upload); (void)hipStreamDestroy(f->upload); }
  slot_free(f->slot[0]);
  slot_free(f->slot[1]);
  delete f;
}

static int fold_check_shape(dspsr_amd_fold* f, const char* who, uint32_t nchan, uint32_t npol, uint32_t ndim, uint32_t nbin)
{
  // ndim 14: the fourth moments of the Stokes parameters (FourthMoment.C:39-42: always one polarisation), fold_moments.hip
  if (ndim == 14 && npol != 1)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: ndim=14 (fourth moments) goes with npol=1, not npol=%u", who, npol);
  if (ndim != 1 && ndim != 2 && ndim != 4 && ndim != 14)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: ndim=%u not in {1,2,4} or 14 with npol 1", who, ndim);
  if (!nchan || !npol || !nbin) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: zero dimension", who);
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_fold_set_shape(dspsr_amd_fold* f, uint32_t nchan, uint32_t npol, uint32_t ndim, uint32_t nbin)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const int rc = fold_check_shape(f, "dspsr_amd_fold_set_shape", nchan, npol, ndim, nbin);
  if (rc != DSPSR_AMD_OK) return rc;
  if (f->bound) {
    if (nchan == f->nchan && npol == f->npol && ndim == f->ndim && nbin == f->nbin) return DSPSR_AMD_OK;
    return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_fold_set_shape: the profile is bound to a caller's buffer of another "
                                              "shape; bind again (dspsr_amd_fold_bind_profile)");
  }
  const size_t need = (size_t)nchan * npol * nbin * ndim;
  if (need != f->profile_floats) {
    // PhaseSeries::mixable/resize on a changed shape starts a new, zeroed profile (Fold.C:495-508)
    (void)hipStreamSynchronize(f->ctx->stream);
    if (f->profile) (void)hipFree(f->profile);
    f->profile = nullptr;
    f->profile_floats = 0;
    if (hipMalloc((void**)&f->profile, need * sizeof(float)) != hipSuccess)
      return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_fold_set_shape: hipMalloc(%zu floats) failed", need);
    f->profile_floats = need;
    (void)hipMemsetAsync(f->profile, 0, need * sizeof(float), f->ctx->stream);
  }
  f->nchan = nchan; f->npol = npol; f->ndim = ndim; f->nbin = nbin;
  f->span = (uint64_t)nbin * ndim;
  return DSPSR_AMD_OK;
}

// Fold::Engine::setup (Fold.C:968-1011) caches output = get_profiles()->get_datptr(0,0) and output_span =
// get_nfloat_span(): the engine folds INTO the device PhaseSeries that Fold::get_output() hands to prepare_output /
// zero / mixable.  The buffer stays the caller's (never freed or zeroed here except through dspsr_amd_fold_zero).
extern "C" int dspsr_amd_fold_bind_profile(dspsr_amd_fold* f, float* profile_dev, uint64_t span_floats, uint32_t nchan,
                                           uint32_t npol, uint32_t ndim, uint32_t nbin)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!profile_dev) {                                      // unbind: back to a library-owned profile of the same shape
    if (f->bound) { f->profile = nullptr; f->bound = false; f->profile_floats = 0; }
    return nchan ? dspsr_amd_fold_set_shape(f, nchan, npol, ndim, nbin) : DSPSR_AMD_OK;
  }
  const int rc = fold_check_shape(f, "dspsr_amd_fold_bind_profile", nchan, npol, ndim, nbin);
  if (rc != DSPSR_AMD_OK) return rc;
  if (span_floats < (uint64_t)nbin * ndim)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fold_bind_profile: span=%llu floats < nbin*ndim=%llu",
                    (unsigned long long)span_floats, (unsigned long long)nbin * ndim);
  if (f->profile && !f->bound) {
    (void)hipStreamSynchronize(f->ctx->stream);
    (void)hipFree(f->profile);
  }
  f->profile = profile_dev;
  f->bound = true;
  f->profile_floats = 0;
  f->span = span_floats;
  f->nchan = nchan; f->npol = npol; f->ndim = ndim; f->nbin = nbin;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_fold_set_nbin(dspsr_amd_fold* f, uint32_t nbin)   // FoldCUDA.cu:64-70
{
  if (!f) return DSPSR_AMD_EINVAL;
  f->current_bin = f->folding_nbin = nbin;
  f->current_hits = 0;
  f->ndat_fold = 0;
  f->binplan.clear();
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_fold_set_ndat(dspsr_amd_fold* f, uint64_t ndat, uint64_t /*idat_start*/)  // :72-82
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (f->binplan.capacity() < ndat) f->binplan.reserve(ndat < (1u << 20) ? ndat : (1u << 20));
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_fold_set_bin(dspsr_amd_fold* f, uint64_t idat, double d_ibin, double /*bins_per_sample*/)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const uint32_t ibin = (uint32_t)d_ibin;                 // FoldCUDA.cu:87
  if (ibin != f->current_bin) {
    if (!f->binplan.empty()) f->binplan.back().hits = f->current_hits;
    RunBin start; start.offset = idat; start.ibin = ibin; start.hits = 0;
    f->binplan.push_back(start);
    f->current_bin = ibin;
    f->current_hits = 0;
  }
  f->ndat_fold++;
  f->current_hits++;
  return DSPSR_AMD_OK;
}

// The plan loop of Fold.C:744-787, the same double recurrence sample by sample (the sums are not associative, so nothing is
// skipped), written so that the loop-carried chain is the one addition: phi -= floor(phi) changes phi only when phi is
// outside [0, 1) (phi - 0.0 == phi), the run-length bookkeeping of set_bin (FoldCUDA.cu:84-113) is inlined and hits[] is
// updated once per run.  At 6 MHz output rates the plan loop is what a block waits for.
// Weights (Fold.C:686-716,746-763): sample idat belongs to weight (idat + weight_idat) / ndatperweight; samples of a zero
// weight are dropped from the plan (binplan = folding_nbin in the reference: not folded, not counted in hits or
// ndat_folded) -- the hook a weighted input (dropped packets, RFI flagging upstream) needs; weights == NULL: none.
static int fold_set_bins_impl(dspsr_amd_fold* f, double phi, double phase_per_sample, uint64_t ndat, uint64_t idat_start,
                              const uint32_t* weights, uint64_t nweights, uint64_t ndatperweight, uint64_t weight_idat,
                              uint32_t* hits_host, uint64_t* ndat_folded)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->folding_nbin) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dsp::Fold::fold nbin not set");
  const double double_nbin = (double)f->folding_nbin;     // Fold.C:719
  const uint32_t nbin = f->folding_nbin;
  uint32_t cur_bin = f->current_bin, cur_hits = f->current_hits;
  uint32_t counted = cur_hits;          // hits of the open run already added to hits_host by an earlier call
  const uint64_t end = idat_start + ndat;
  uint64_t folded = 0, iweight = 0, idat_nextweight = ~0ull;
  bool bad = false;
  if (weights && ndatperweight) {                         // Fold.C:686-716
    iweight = (idat_start + weight_idat) / ndatperweight;
    idat_nextweight = (iweight + 1) * ndatperweight - weight_idat;
    if (iweight >= nweights)
      return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dsp::Fold::fold iweight=%llu >= nweight=%llu", (unsigned long long)iweight,
                      (unsigned long long)nweights);
    bad = weights[iweight] == 0;
  }
  // cur_bin == nbin (the value set_nbin leaves, FoldCUDA.cu:64-70) means "no run open": the last entry of the plan, if
  // any, already has its final hits
  auto close_run = [&]() {              // a dropped sample ends the open run: the next kept sample starts a new one
    if (cur_bin < nbin) {
      if (!f->binplan.empty()) f->binplan.back().hits = cur_hits;
      if (hits_host) hits_host[cur_bin] += cur_hits - counted;
    }
    cur_bin = nbin; cur_hits = 0; counted = 0;
  };
  // (a run costs the short cut about 70 ns, a sample of the loop 1 ns: it pays from runs of a hundred samples on -- the headline's
  //  34-sample runs keep the loop)
  if ((!weights || !ndatperweight) && phase_per_sample >= 0.0 && phase_per_sample * double_nbin * 128.0 <= 1.0) {
    // No weights, long runs: the plan run by run (host_prep.cpp fold_plan_run: the values of the recurrence below without walking the samples of
    // a run -- a 50 MHz channel's block is 10 M samples and 1100 runs).  Same bookkeeping as the sample loop: a new run where the bin
    // changes, hits[] once per run.
    uint64_t idat = idat_start;
    while (idat < end) {
      uint32_t ibin;
      uint64_t n = fold_plan_run(&phi, phase_per_sample, double_nbin, end - idat, &ibin);
      if (ibin >= nbin) {
        f->current_bin = cur_bin; f->current_hits = cur_hits;
        return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dsp::Fold::fold ibin=%u >= nbin=%u", ibin, nbin);
      }
      if (ibin != cur_bin) {
        if (cur_bin < nbin) {
          if (!f->binplan.empty()) f->binplan.back().hits = cur_hits;
          if (hits_host) hits_host[cur_bin] += cur_hits - counted;
        }
        RunBin start; start.offset = idat; start.ibin = ibin; start.hits = 0;
        f->binplan.push_back(start);
        cur_bin = ibin;
        cur_hits = 0;
        counted = 0;
      }
      cur_hits += (uint32_t)n;
      folded += n;
      idat += n;
    }
  } else
  for (uint64_t idat = idat_start; idat < end; idat++) {
    if (idat >= idat_nextweight) {                        // Fold.C:746-763
      iweight++;
      if (iweight >= nweights) {
        f->current_bin = cur_bin; f->current_hits = cur_hits;
        return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dsp::Fold::fold iweight=%llu >= nweight=%llu", (unsigned long long)iweight,
                        (unsigned long long)nweights);
      }
      bad = weights[iweight] == 0;
      idat_nextweight += ndatperweight;
    }
    if (!(phi >= 0.0 && phi < 1.0)) phi -= floor(phi);
    const uint32_t ibin = (uint32_t)(phi * double_nbin);
    phi += phase_per_sample;
    if (ibin >= nbin) {
      f->current_bin = cur_bin; f->current_hits = cur_hits;
      return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dsp::Fold::fold ibin=%u >= nbin=%u", ibin, nbin);
    }
    if (bad) {
      close_run();
      continue;
    }
    if (ibin != cur_bin) {                // set_bin: a new run starts
      if (cur_bin < nbin) {               // (an open run ends here)
        if (!f->binplan.empty()) f->binplan.back().hits = cur_hits;
        if (hits_host) hits_host[cur_bin] += cur_hits - counted;
      }
      RunBin start; start.offset = idat; start.ibin = ibin; start.hits = 0;
      f->binplan.push_back(start);
      cur_bin = ibin;
      cur_hits = 0;
      counted = 0;
    }
    cur_hits++;
    folded++;
  }
  if (hits_host && cur_bin < nbin) hits_host[cur_bin] += cur_hits - counted;
  f->ndat_fold += folded;
  f->current_bin = cur_bin;
  f->current_hits = cur_hits;
  if (ndat_folded) *ndat_folded = folded;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_fold_set_bins(dspsr_amd_fold* f, double phi, double phase_per_sample, uint64_t ndat,
                                       uint64_t idat_start, uint32_t* hits_host, uint64_t* ndat_folded)
{
  return fold_set_bins_impl(f, phi, phase_per_sample, ndat, idat_start, nullptr, 0, 0, 0, hits_host, ndat_folded);
}

extern "C" int dspsr_amd_fold_set_bins_weighted(dspsr_amd_fold* f, double phi, double phase_per_sample, uint64_t ndat,
                                                uint64_t idat_start, const uint32_t* weights_host, uint64_t nweights,
                                                uint64_t ndatperweight, uint64_t weight_idat, uint32_t* hits_host,
                                                uint64_t* ndat_folded)
{
  if (weights_host && !ndatperweight) return DSPSR_AMD_EINVAL;
  return fold_set_bins_impl(f, phi, phase_per_sample, ndat, idat_start, weights_host, nweights, ndatperweight, weight_idat,
                            hits_host, ndat_folded);
}

extern "C" uint64_t dspsr_amd_fold_get_ndat_folded(const dspsr_amd_fold* f) { return f ? f->ndat_fold : 0; }
extern "C" float* dspsr_amd_fold_profiles_dev(dspsr_amd_fold* f) { return f ? f->profile : nullptr; }

extern "C" int dspsr_amd_fold_zero(dspsr_amd_fold* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->profile) return DSPSR_AMD_OK;
  const size_t row = (size_t)f->nbin * f->ndim * sizeof(float);
  hipError_t e = f->span == (uint64_t)f->nbin * f->ndim
                     ? hipMemsetAsync(f->profile, 0, row * f->nchan * f->npol, f->ctx->stream)
                     : hipMemset2DAsync(f->profile, f->span * sizeof(float), 0, row, (size_t)f->nchan * f->npol, f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_fold_zero: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

// The closed plan of `f` on its way to the device in the engine's next slot, over the chunk grid [first, last): the dense
// table of k_fold_dense (aux) when try_dense, the plan fits it (plan_scan) and no run is a LONG one; the intervals bucketed by
// phase bin (bin_start / iv: the walk kernels, the hit count of a zeroed input) when there is no table or the caller wants
// them all the same.  Nothing is uploaded that no kernel reads.  The compute stream waits for the copies; the caller
// launches, calls slot_submit and clears the plan.
struct SentPlan { PlanSlot* slot; uint32_t max_run; bool dense; };
static int plan_send(dspsr_amd_fold* f, const char* who, uint64_t first, uint64_t last, bool try_dense, bool want_iv, SentPlan* out)
{
  dspsr_amd_ctx* ctx = f->ctx;
  const RunBin* runs = f->binplan.data();
  const size_t niv = f->binplan.size(), nbin1 = (size_t)f->nbin + 1;
  size_t ntab = 0;
  bool one_per_chunk = false;
  out->max_run = plan_scan(runs, niv, f->nbin, (uint64_t)f->nchan * f->npol * f->ndim, try_dense, first, last, f->cursor, &ntab, &one_per_chunk);
  out->dense = one_per_chunk && out->max_run < FOLD_LONG_RUN;
  const bool need_iv = !out->dense || want_iv;
  const int rc = slot_acquire(f, who, &out->slot);
  if (rc != DSPSR_AMD_OK) return rc;
  PlanSlot& sl = *out->slot;
  if (!slot_reserve(sl, nbin1, niv, out->dense ? ntab : 0)) return ctx_fail(ctx, DSPSR_AMD_ENOMEM, "%s: plan allocation failed", who);
  if (need_iv) plan_bucket(runs, niv, f->nbin, sl.h_bin_start, sl.h_iv, f->cursor);
  if (out->dense) plan_dense_fill(runs, niv, f->nbin, first, sl.h_aux, ntab);
  const PlanCopy pc[3] = {{sl.d_bin_start, sl.h_bin_start, need_iv ? nbin1 * sizeof(uint32_t) : 0},
                          {sl.d_iv, sl.h_iv, need_iv ? niv * sizeof(Interval) : 0},
                          {sl.d_aux, sl.h_aux, out->dense ? ntab * sizeof(uint32_t) : 0}};
  const hipError_t e = plan_upload(f, sl, pc, 3);
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "%s: plan copy: %s", who, hipGetErrorString(e));
  return fold_plan_wait(f, &sl);
}

// sample span covered by a closed plan (intervals are time ordered)
static void plan_span(const dspsr_amd_fold* f, uint64_t* first, uint64_t* last)
{
  *first = f->binplan.front().offset;
  *last = f->binplan.back().offset + f->binplan.back().hits;
}

// (fold_internal.h; the plan is not empty: the caller has looked)
int fold_plan_to_device(dspsr_amd_fold* f, const char* who, PlanSlot** slot, uint64_t* first, uint64_t* last, uint32_t* max_run)
{
  plan_close(f);
  plan_span(f, first, last);
  *first -= *first % 4;                                // keeps 16-byte alignment of the chunk loads for any ndim
  SentPlan sp;
  const int rc = plan_send(f, who, *first, *last, false, true, &sp);
  if (rc != DSPSR_AMD_OK) return rc;
  f->binplan.clear();
  *slot = sp.slot;
  *max_run = sp.max_run;
  return DSPSR_AMD_OK;
}

// The instantiations <ND, NR> of the chunk kernels (floats per sample, rows per workgroup: fold_plan.h FoldShape nd, nr): fn is
// called with the pair as a type.
template <int ND, int NR> struct FoldInstance { static constexpr int nd = ND, nr = NR; };
template <class Fn>
static void fold_instance(uint32_t ndim, uint32_t nrw, Fn&& fn)
{
  if (ndim == 4) fn(FoldInstance<4, 1>());
  else if (ndim == 2 && nrw == 2) fn(FoldInstance<2, 2>());
  else if (ndim == 2) fn(FoldInstance<2, 1>());
  else if (nrw == 4) fn(FoldInstance<1, 4>());
  else fn(FoldInstance<1, 1>());
}

static int fold_fold_impl(dspsr_amd_fold* f, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                          uint32_t* hits_dev);

extern "C" int dspsr_amd_fold_fold(dspsr_amd_fold* f, const float* in_dev, uint64_t in_chan_stride,
                                   uint64_t in_pol_stride)
{
  // a 14-shape folds ndim 14 rows, the output of a FourthMoment operation (fold_moments.hip, stream loader)
  if (f && f->ndim == 14) return fold_moments_run(f, in_dev, in_chan_stride, false, "dspsr_amd_fold_fold");
  return fold_fold_impl(f, in_dev, in_chan_stride, in_pol_stride, nullptr);
}

extern "C" int dspsr_amd_fold_fold_zeroed(dspsr_amd_fold* f, const float* in_dev, uint64_t in_chan_stride,
                                          uint64_t in_pol_stride, uint32_t* hits_dev)
{
  if (!hits_dev) return DSPSR_AMD_EINVAL;
  if (f && f->ndim == 14)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fold_fold_zeroed: not built for fourth moments (npol 1 x ndim 14)");
  return fold_fold_impl(f, in_dev, in_chan_stride, in_pol_stride, hits_dev);
}

static int fold_fold_impl(dspsr_amd_fold* f, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                          uint32_t* hits_dev)
{
  if (!f || !in_dev) return DSPSR_AMD_EINVAL;
  dspsr_amd_ctx* ctx = f->ctx;
  if (!f->profile) return ctx_fail(ctx, DSPSR_AMD_ESTATE, "dspsr_amd_fold_fold: set_shape not called");
  if (f->folding_nbin != f->nbin)    // Fold.C:806-809
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dsp::Fold::fold folding_nbin != output->nbin (%u != %u)",
                    f->folding_nbin, f->nbin);
  if (f->binplan.empty()) return DSPSR_AMD_OK;             // send_binplan :160-161
  plan_close(f);
  const uint32_t nbin = f->nbin;
  uint64_t first, last;
  plan_span(f, &first, &last);
  first -= first % 4;                                  // keeps 16-byte alignment of the chunk loads for any ndim
  const bool aligned = ((uintptr_t)in_dev % 16 == 0) && (in_chan_stride % 4 == 0) && (in_pol_stride % 4 == 0);
  SentPlan sp;
  int rc = plan_send(f, "dspsr_amd_fold_fold", first, last, fold_takes_chunks(aligned, nbin), hits_dev != nullptr, &sp);
  if (rc != DSPSR_AMD_OK) return rc;
  PlanSlot& sl = *sp.slot;
  const FoldShape s = fold_shape(aligned, f->nchan, f->npol, f->ndim, nbin, first, last, sp.max_run, sp.dense, ctx->ncu);
  if (s.family == FOLD_LONG) {
    const size_t need = (size_t)s.nseg * f->npol * f->nchan * nbin * f->ndim;
    if (!grow_device_buffer(ctx->stream, f->part, f->part_floats, need))
      return ctx_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_fold_fold: hipMalloc of %zu partial-sum floats failed", need);
  }
  const dim3 grid(s.grid[0], s.grid[1], s.grid[2]), block(s.threads);
  const uint32_t cps = (uint32_t)s.seg_len;
  fold_instance(s.nd, s.nr, [&](auto inst) {
    constexpr int ND = decltype(inst)::nd, NR = decltype(inst)::nr;
    if (s.family == FOLD_DIRECT)                           // (NR is 1)
      hipLaunchKernelGGL(k_fold_direct<ND>, grid, block, 0, ctx->stream, in_dev, in_chan_stride, in_pol_stride, f->profile, f->span,
                         nbin, sl.d_bin_start, sl.d_iv);
    else if (s.family == FOLD_DENSE)
      hipLaunchKernelGGL((k_fold_dense<ND, NR>), grid, block, s.lds, ctx->stream, in_dev, in_chan_stride, in_pol_stride, f->profile,
                         f->span, nbin, sl.d_aux, first, last);
    else if (s.family == FOLD_LONG)
      hipLaunchKernelGGL((k_fold_chunked<ND, true, NR>), grid, block, s.lds, ctx->stream, in_dev, in_chan_stride, in_pol_stride,
                         f->profile, f->span, nbin, sl.d_bin_start, sl.d_iv, first, last, f->part, cps);
    else
      hipLaunchKernelGGL((k_fold_chunked<ND, false, NR>), grid, block, s.lds, ctx->stream, in_dev, in_chan_stride, in_pol_stride,
                         f->profile, f->span, nbin, sl.d_bin_start, sl.d_iv, first, last, f->part, cps);
  });
  if (s.family == FOLD_LONG && (rc = fold_combine_partials(f, "dspsr_amd_fold_fold", f->part, s.nseg, 0, f->nchan)) != DSPSR_AMD_OK) return rc;
  if (hits_dev)     // per-channel hits of a zeroed input: polarisation 0, first float of every planned sample
    hipLaunchKernelGGL(k_fold_count_hits, dim3((nbin + 255) / 256, f->nchan), dim3(256), 0, ctx->stream, in_dev, in_chan_stride, f->ndim,
                       hits_dev, nbin, sl.d_bin_start, sl.d_iv);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_fold_fold: %s", hipGetErrorString(e));
  if (slot_submit(f, "dspsr_amd_fold_fold", sl) != DSPSR_AMD_OK) return DSPSR_AMD_EHIP;
  f->binplan.clear();
  return DSPSR_AMD_OK;
}

// One launch of k_fold_many over the group g[0 .. n) (n <= FOLD_MANY_MAX), every plan pending, exact order (no LONG run), rows
// 16-byte aligned and nbin within the chunk kernels: each plan goes through its own double-buffered slot as in fold_fold_impl.
static int fold_many_group(dspsr_amd_fold* const* g, uint32_t n, const float* in_dev, uint64_t in_chan_stride,
                           uint64_t in_pol_stride)
{
  dspsr_amd_fold* f0 = g[0];
  dspsr_amd_ctx* ctx = f0->ctx;
  // the chunk grid of the group starts at the first sample of any plan (rounded down: 16-byte aligned chunk loads) and ends
  // with the last one
  uint64_t first = ~0ull, last = 0;
  for (uint32_t k = 0; k < n; k++) {
    dspsr_amd_fold* f = g[k];
    plan_close(f);
    uint64_t a, b;
    plan_span(f, &a, &b);
    if (a < first) first = a;
    if (b > last) last = b;
  }
  first -= first % 4;
  FoldManyArgs args;
  ::memset((void*)&args, 0, sizeof(args));
  PlanSlot* used[FOLD_MANY_MAX];
  uint32_t nslot = 0;
  for (uint32_t k = 0; k < n; k++) {
    dspsr_amd_fold* f = g[k];
    const uint32_t nbin = f->nbin;
    SentPlan sp;                   // the dense table over the group's chunk grid, or the bucketed plan
    const int rc = plan_send(f, "dspsr_amd_fold_fold_many", first, last, true, false, &sp);
    if (rc != DSPSR_AMD_OK) return rc;
    PlanSlot& sl = *sp.slot;
    FoldManyPlan& p = args.p[k];
    p.prof = f->profile;
    p.span = f->span;
    p.bin_start = sl.d_bin_start;
    p.iv = sl.d_iv;
    p.tab = sp.dense ? sl.d_aux : nullptr;
    p.nbin = nbin;
    p.slot0 = nslot;
    nslot += nbin;
    used[k] = &sl;
  }
  args.nplan = n;
  args.nslot = nslot;
  const FoldShape s = fold_many_shape(f0->nchan, f0->npol, f0->ndim, nslot, ctx->ncu);
  fold_instance(s.nd, s.nr, [&](auto inst) {
    hipLaunchKernelGGL((k_fold_many<decltype(inst)::nd, decltype(inst)::nr>), dim3(s.grid[0], s.grid[1], s.grid[2]), dim3(s.threads),
                       s.lds, ctx->stream, in_dev, in_chan_stride, in_pol_stride, args, first, last);
  });
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_fold_fold_many: %s", hipGetErrorString(e));
  for (uint32_t k = 0; k < n; k++) {
    const int rc = slot_submit(g[k], "dspsr_amd_fold_fold_many", *used[k]);
    g[k]->binplan.clear();
    if (rc != DSPSR_AMD_OK) return rc;
  }
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_fold_fold_many(dspsr_amd_fold* const* folds, uint32_t nfold, const float* in_dev,
                                        uint64_t in_chan_stride, uint64_t in_pol_stride, uint32_t* nshared)
{
  if (nshared) *nshared = 0;
  if (nfold == 0) return DSPSR_AMD_OK;
  if (!folds || !in_dev) return DSPSR_AMD_EINVAL;
  // every refusal comes before any plan is touched
  for (uint32_t i = 0; i < nfold; i++) {
    dspsr_amd_fold* f = folds[i];
    if (!f) return DSPSR_AMD_EINVAL;
    for (uint32_t j = 0; j < i; j++)
      if (folds[j] == f) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fold_fold_many: fold %u given twice", i);
    if (f->ctx != folds[0]->ctx) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fold_fold_many: fold %u of another context", i);
    if (f->ndim == 14)
      return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fold_fold_many: fold %u folds fourth moments (npol 1 x ndim 14): not built for a shared launch", i);
    if (f->nchan != folds[0]->nchan || f->npol != folds[0]->npol || f->ndim != folds[0]->ndim)
      return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fold_fold_many: fold %u has another nchan / npol / ndim", i);
    if (!f->profile) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_fold_fold_many: fold %u: set_shape not called", i);
    if (f->folding_nbin != f->nbin)    // Fold.C:806-809
      return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dsp::Fold::fold folding_nbin != output->nbin (%u != %u), fold %u",
                      f->folding_nbin, f->nbin, i);
  }
  // the rules of fold_fold_impl: exact-order plans of the chunk kernels share the launch; LONG runs and k_fold_direct (unaligned
  // rows, nbin beyond the chunk kernels) go through the single-fold code; empty plans are skipped
  const bool aligned = ((uintptr_t)in_dev % 16 == 0) && (in_chan_stride % 4 == 0) && (in_pol_stride % 4 == 0);
  std::vector<dspsr_amd_fold*> shared;
  for (uint32_t i = 0; i < nfold; i++) {
    dspsr_amd_fold* f = folds[i];
    if (f->binplan.empty()) continue;
    if (fold_takes_chunks(aligned, f->nbin) && fold_plan_max_run(f) < FOLD_LONG_RUN) {
      shared.push_back(f);
      continue;
    }
    const int rc = fold_fold_impl(f, in_dev, in_chan_stride, in_pol_stride, nullptr);
    if (rc != DSPSR_AMD_OK) return rc;
  }
  // a lone exact-order plan gains nothing from sharing: the single-fold kernels fold it with the same sums, faster
  if (shared.size() == 1) return fold_fold_impl(shared[0], in_dev, in_chan_stride, in_pol_stride, nullptr);
  // launches of at most FOLD_MANY_MAX plans, their sizes balanced (9 plans: 5 + 4), so that no launch holds a single plan
  const size_t ngroup = (shared.size() + FOLD_MANY_MAX - 1) / FOLD_MANY_MAX;
  for (size_t g = 0, i = 0; g < ngroup; g++) {
    const size_t end = shared.size() * (g + 1) / ngroup;
    const uint32_t n = (uint32_t)(end - i);
    const int rc = fold_many_group(shared.data() + i, n, in_dev, in_chan_stride, in_pol_stride);
    if (rc != DSPSR_AMD_OK) return rc;
    if (nshared) *nshared += n;
    i = end;
  }
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_fold_synch(dspsr_amd_fold* f, float* profile_host)   // FoldCUDA.cu:127-152
{
  if (!f || !profile_host) return DSPSR_AMD_EINVAL;
  if (!f->profile) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_fold_synch: no profile");
  const size_t row = (size_t)f->nbin * f->ndim * sizeof(float);      // host copy is packed [chan][pol][nbin][ndim]
  hipError_t e = hipMemcpy2DAsync(profile_host, row, f->profile, f->span * sizeof(float), row, (size_t)f->nchan * f->npol,
                                  hipMemcpyDeviceToHost, f->ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_fold_synch: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

int fold_build_part_plan(dspsr_amd_fold* f, uint32_t nkeep, uint32_t npart, const uint32_t** d_start,
                         const Interval** d_iv, PlanSlot** slot)
{
  dspsr_amd_ctx* ctx = f->ctx;
  plan_close(f);
  const RunBin* runs = f->binplan.data();
  const size_t nrun = f->binplan.size();
  PartPlanSize sz;
  uint64_t beyond = 0;
  if (!part_plan_count(runs, nrun, nkeep, npart, f->nbin, f->cursor, &sz, &beyond))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "fused fold: plan sample %llu lies beyond the %u parts of this call",
                    (unsigned long long)beyond, npart);
  PlanSlot* sl = nullptr;
  const int rc = slot_acquire(f, "fused fold", &sl);
  if (rc != DSPSR_AMD_OK) return rc;
  if (!slot_reserve(*sl, sz.nwords, sz.npiece ? sz.npiece : 1, 0))
    return ctx_fail(ctx, DSPSR_AMD_ENOMEM, "fused fold: plan allocation failed");
  part_plan_fill(runs, nrun, nkeep, npart, f->nbin, f->cursor, sl->h_bin_start, sl->h_iv);
  const PlanCopy pc[2] = {{sl->d_bin_start, sl->h_bin_start, sz.nwords * sizeof(uint32_t)}, {sl->d_iv, sl->h_iv, sz.npiece * sizeof(Interval)}};
  const hipError_t e = plan_upload(f, *sl, pc, 2);      // the caller waits (fold_plan_wait) in front of the kernel that reads it
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "fused fold: plan copy: %s", hipGetErrorString(e));
  f->binplan.clear();
  *d_start = sl->d_bin_start;
  *d_iv = sl->d_iv;
  *slot = sl;
  return DSPSR_AMD_OK;
}

int fold_combine_partials(dspsr_amd_fold* f, const char* who, const float* part, uint32_t nseg, uint32_t chan0, uint32_t nchan)
{
  // profile rows [chan0, chan0 + nchan) += partial profiles of the runs 1 .. nseg of a segmented fused launch (packed
  // [seg][chan - chan0][nbin][ndim], npol 1), in run order
  const uint32_t nrow = nchan * f->npol;
  const uint64_t n = (uint64_t)nrow * f->nbin * f->ndim;
  uint32_t gx = (uint32_t)((n + 255) / 256);
  if (gx > 4 * f->ctx->ncu) gx = 4 * f->ctx->ncu;
  hipLaunchKernelGGL(k_fold_combine, dim3(gx), dim3(256), 0, f->ctx->stream, f->profile + (uint64_t)chan0 * f->npol * f->span, f->span,
                     part, nrow, f->nbin * f->ndim, nseg);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

int fold_build_segment_plan(dspsr_amd_fold* f, uint64_t ndat, uint32_t seg, bool* ok, const uint32_t** d_run_off,
                            const uint32_t** d_blk_first, const uint32_t** d_bin_start, const Interval** d_iv, PlanSlot** slot)
{
  dspsr_amd_ctx* ctx = f->ctx;
  *ok = false;
  const size_t nrun = f->binplan.size();
  if (!segment_plan_qualifies(f->binplan.data(), nrun, f->current_hits, ndat, seg)) return DSPSR_AMD_OK;
  plan_close(f);
  const uint32_t nbin = f->nbin;
  PlanSlot* sl = nullptr;
  const int rc = slot_acquire(f, "fused fold", &sl);
  if (rc != DSPSR_AMD_OK) return rc;
  const size_t naux = nrun + 1 + segment_plan_nblk(ndat);
  if (!slot_reserve(*sl, (size_t)nbin + 1, nrun, naux)) return ctx_fail(ctx, DSPSR_AMD_ENOMEM, "fused fold: plan allocation failed");
  segment_plan_fill(f->binplan.data(), nrun, nbin, ndat, sl->h_aux, sl->h_aux + nrun + 1, sl->h_bin_start, sl->h_iv, f->cursor);
  const PlanCopy pc[3] = {{sl->d_aux, sl->h_aux, naux * sizeof(uint32_t)}, {sl->d_bin_start, sl->h_bin_start, ((size_t)nbin + 1) * sizeof(uint32_t)},
                          {sl->d_iv, sl->h_iv, nrun * sizeof(Interval)}};
  const hipError_t e = plan_upload(f, *sl, pc, 3);      // the caller waits (fold_plan_wait) in front of the kernel that reads it
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "fused fold: plan copy: %s", hipGetErrorString(e));
  f->binplan.clear();
  *d_run_off = sl->d_aux;
  *d_blk_first = sl->d_aux + nrun + 1;
  *d_bin_start = sl->d_bin_start;
  *d_iv = sl->d_iv;
  *slot = sl;
  *ok = true;
  return DSPSR_AMD_OK;
}

int fold_segment_combine(dspsr_amd_fold* f, const float* msum, uint32_t chan0, uint32_t nchan, uint32_t npart, uint32_t nkeep,
                         uint32_t nfilt_pos, int logTt, int logMa, int logMb, const uint32_t* d_bin_start, const Interval* d_iv)
{
  // (profile of npol 1 x ndim 4, rows 16-byte aligned: checked by the caller)
  hipLaunchKernelGGL(k_fold_segsum, dim3((f->nbin + 255) / 256, nchan), dim3(256), 0, f->ctx->stream,
                     f->profile + (uint64_t)chan0 * f->span, f->span, f->nbin, (const float4*)msum, npart, nkeep, nfilt_pos, logTt, logMa,
                     logMb, d_bin_start, d_iv);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "fused fold: segment combine: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
