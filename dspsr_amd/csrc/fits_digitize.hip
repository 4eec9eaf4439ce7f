// PSRFITS search-mode output stage for gfx950: dsp::FITSDigitizer::rescale_pack, FPT branch (Kernel/Formats/fits/FITSDigitizer.C),
// the back half of digifits (Signal/General/LoadToFITS.C:519-553).  It is NOT dsp::Rescale followed by dsp::SigProcDigitizer:
//
//   measure_scale (:178-321): per (pol, chan) the sums of x and of the float-rounded x*x over exactly ONE block of nsblk samples, in
//       double; offset = mean and scale = standard deviation from the block alone (nblock 1), from the rows of a ring of nblock
//       blocks while it fills, or from the running values with the newest block added and the block at `old_idx` subtracted once
//       the ring is full; `constant` keeps the first block's pair.
//   rescale_pack (:602-661): m_scale = float(1/scale), m_offset = float(offset); tmp = (x - m_offset) * m_scale in float;
//       int(tmp * digi_scale + digi_mean + 0.5) with digi_sigma 8 (:14-45), clipped to [0, 2^nbit - 1]; sample idat*nchan*npol +
//       ipol*nchan + ichan (TPF), sub-byte samples MOST significant bits first.
//   get_scales (:675-699): DAT_SCL = scale / digi_scale, DAT_OFFS = offset, as floats, in output channel order.
//
// The reference runs this on the host behind a device-to-host copy of the rows (LoadToFITS.C:441-450); here the rows stay in HBM and
// a pack() is three launches on the context's stream: k_fits_sums (fixed-order tree per row, as k_rescale_sums_fpt), k_fits_update
// (one thread per (pol, output channel): the ring, offset / scale in double, the float pair the pack applies, DAT_SCL / DAT_OFFS)
// and k_fits_pack (the 64 x 64 LDS turn of k_digitize_fpt).  No host synchronisation, no atomics: rescale_idx and rescale_counter
// do not depend on data and stay host integers.  The order of the double additions inside a row is the only licensed difference
// from the reference; on data whose sums are exact in double every byte and float equals the reference's.
#include <math.h>

#include "engine_internal.h"

namespace dspsr_amd {

constexpr uint32_t FITS_SLICE = 4096;          // samples per workgroup of the sums pass

__device__ __forceinline__ uint32_t fits_channel(uint32_t k, const uint32_t nchan, const int flip_band, const int swap_band)
{
  if (swap_band) k = (k + nchan / 2) % nchan;  // ChannelSort (FITSDigitizer.C:116-145), taken as k_digitize_fpt takes
  if (flip_band) k = nchan - k - 1;            // SigProcDigitizer's identical map
  return k;
}

// partial sums of one time slice of one row: block (x: slice, y: row = chan * npol + pol); fixed-order tree in LDS (deterministic);
// the partials are indexed as the reference indexes its arrays, ipol * nchan + ichan
__global__ __launch_bounds__(256) void k_fits_sums(const float* __restrict__ in, const uint64_t ics, const uint64_t ips, const uint32_t nchan,
                                                   const uint32_t npol, const uint32_t ndat, double* __restrict__ part_sum,
                                                   double* __restrict__ part_sq)
{
  __shared__ double ss[256], sq[256];
  const uint32_t chan = blockIdx.y / npol, pol = blockIdx.y % npol, ncol = nchan * npol;
  const float* __restrict__ x = in + chan * ics + pol * ips;
  const uint32_t i0 = blockIdx.x * FITS_SLICE, i1 = ndat - i0 < FITS_SLICE ? ndat : i0 + FITS_SLICE;
  double s = 0.0, q = 0.0;
  for (uint32_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float v = x[i];
    s += (double)v;
    q += (double)__fmul_rn(v, v);                        // the reference squares in float and accumulates in double (:237)
  }
  ss[threadIdx.x] = s; sq[threadIdx.x] = q;
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (threadIdx.x < w) { ss[threadIdx.x] += ss[threadIdx.x + w]; sq[threadIdx.x] += sq[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint64_t o = (uint64_t)blockIdx.x * ncol + pol * nchan + chan;
    part_sum[o] = ss[0]; part_sq[o] = sq[0];
  }
}

enum { FITS_SINGLE = 0, FITS_FILLING = 1, FITS_FULL = 2, FITS_KEEP = 3 };

// measure_scale behind the sums (:252-320) and get_scales (:675-699).  One thread per (pol, OUTPUT channel k): it owns input channel
// ChannelSort(k) -- the map is a bijection, so every column is updated once.  Products are rounded before they are added, as the host
// code's are (no fma contraction).  regime FITS_KEEP (`constant` after the first block, :181): the spectrum stays, the scales leave.
__global__ __launch_bounds__(256) void k_fits_update(const double* __restrict__ part_sum, const double* __restrict__ part_sq, const uint32_t nslice,
                                                     const uint32_t nchan, const uint32_t npol, const int regime, const uint32_t idx,
                                                     const uint32_t old_idx, const uint32_t nrow, const double recip,
                                                     double* __restrict__ ring_sum, double* __restrict__ ring_sq, double* __restrict__ offset,
                                                     double* __restrict__ scale, float* __restrict__ m_offset, float* __restrict__ m_scale,
                                                     const float digi_scale, const int flip_band, const int swap_band,
                                                     float* __restrict__ dat_scl, float* __restrict__ dat_offs)
{
  const uint32_t ncol = nchan * npol, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= ncol) return;
  const uint32_t ipol = o / nchan, i = ipol * nchan + fits_channel(o % nchan, nchan, flip_band, swap_band);
  if (regime != FITS_KEEP) {
    double ft = 0.0, fts = 0.0;                            // :194-198, :240-241
    for (uint32_t s = 0; s < nslice; s++) { ft += part_sum[(uint64_t)s * ncol + i]; fts += part_sq[(uint64_t)s * ncol + i]; }
    ring_sum[(uint64_t)idx * ncol + i] = ft;
    ring_sq[(uint64_t)idx * ncol + i] = fts;
    double off, sc;
    if (regime == FITS_FULL) {                             // :308-318
      const double old_offset = offset[i], old_scale = scale[i];
      const double old_ft = ring_sum[(uint64_t)old_idx * ncol + i], old_fts = ring_sq[(uint64_t)old_idx * ncol + i];
      off = old_offset + __dmul_rn(ft - old_ft, recip);
      sc = sqrt(__dsub_rn(__dmul_rn(old_scale, old_scale), __dmul_rn(off, off)) + __dmul_rn(old_offset, old_offset) +
                __dmul_rn(fts - old_fts, recip));
    } else {
      if (regime == FITS_FILLING) {                        // :272-291: the rows so far, added in row order from zero
        ft = 0.0; fts = 0.0;
        for (uint32_t r = 0; r < nrow; r++) { ft += ring_sum[(uint64_t)r * ncol + i]; fts += ring_sq[(uint64_t)r * ncol + i]; }
      }
      off = __dmul_rn(ft, recip);                          // :259-260, :297-298
      sc = sqrt(__dsub_rn(__dmul_rn(fts, recip), __dmul_rn(off, off)));
    }
    offset[i] = off;
    scale[i] = sc;
    m_scale[i] = (float)(1.0 / sc);                        // :621-622
    m_offset[i] = (float)off;
  }
  dat_scl[o] = (float)(scale[i] / (double)digi_scale);     // :693 (a double divided by a float)
  dat_offs[o] = (float)offset[i];
}

// rescale_pack, FPT branch (:612-660): a block turns 64 time samples x 64 output channels of one polarisation through LDS -- rows are
// read along time (coalesced), bytes leave along the channels, in the TPF order of the file.
__global__ __launch_bounds__(256) void k_fits_pack(const float* __restrict__ in, const uint64_t ics, const uint64_t ips, uint8_t* __restrict__ out,
                                                   const uint32_t ndat, const uint32_t nchan, const uint32_t npol, const uint32_t nbit,
                                                   const float* __restrict__ m_offset, const float* __restrict__ m_scale,
                                                   const float digi_scale, const float digi_mean, const int digi_max, const int flip_band,
                                                   const int swap_band)
{
  __shared__ float tile[64][65];
  const uint32_t k0 = blockIdx.x * 64, ipol = blockIdx.z;
  const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;       // read: tx = time, ty + 4 j = channel of the tile
  const uint32_t spb = 8 / nbit, units = 64 / spb;                   // bytes of the tile per time sample
  // (time tiles beyond the grid's y limit: the block walks on; the trip count is the same for every thread of a block)
  for (uint32_t t0 = blockIdx.y * 64; t0 < ndat; t0 += gridDim.y * 64) {
    for (uint32_t j = 0; j < 16; j++) {
      const uint32_t k = k0 + ty + 4 * j;
      float v = 0.f;
      if (k < nchan && t0 + tx < ndat) {
        const uint32_t ic = fits_channel(k, nchan, flip_band, swap_band);
        const float x = in[ic * ics + ipol * ips + t0 + tx];
        v = __fmul_rn(__fsub_rn(x, m_offset[ipol * nchan + ic]), m_scale[ipol * nchan + ic]);        // :627
      }
      tile[ty + 4 * j][tx] = v;
    }
    __syncthreads();
    auto level = [&](const float tmp) {
      // :628  float multiply, float add, then + 0.5 in double (the literal is a double), truncation; out-of-range and NaN
      // conversions yield INT_MIN on the reference's x86 hosts (cvttsd2si), i.e. clip to digi_min = 0
      const double d = (double)__fadd_rn(__fmul_rn(tmp, digi_scale), digi_mean) + 0.5;
      int r = (d >= 2147483648.0 || d <= -2147483649.0 || d != d) ? (int)0x80000000 : (int)d;
      r = r > digi_max ? digi_max : r;                               // :632
      return r < 0 ? 0 : r;
    };
    for (uint32_t u = threadIdx.x; u < 64 * units; u += 256) {       // write: consecutive threads, consecutive bytes of a time sample
      const uint32_t tt = u / units, w = u % units, k = k0 + w * spb;
      if (k >= nchan || t0 + tt >= ndat) continue;
      uint32_t byte = 0;
      for (uint32_t j = 0; j < spb; j++) byte |= (uint32_t)level(tile[w * spb + j][tt]) << ((spb - j - 1) * nbit);   // :646: MSB first
      out[((uint64_t)(t0 + tt) * nchan * npol + (uint64_t)ipol * nchan + k) / spb] = (uint8_t)byte;
    }
    __syncthreads();                                                 // the tile is free for the next time slice
  }
}

}  // namespace dspsr_amd

using namespace dspsr_amd;

struct dspsr_amd_fits_digitizer {
  dspsr_amd_ctx* ctx;
  uint32_t nchan, npol, ncol, nbit, nsblk, nblock, nslice;
  bool constant;
  int flip_band, swap_band;
  float digi_scale, digi_mean;
  int digi_max;
  uint32_t rescale_idx = 0, rescale_counter = 0;       // host integers, as the reference's (:54-55)
  double *ring_sum = nullptr, *ring_sq = nullptr, *offset = nullptr, *scale = nullptr, *part_sum = nullptr, *part_sq = nullptr;
  float *m_offset = nullptr, *m_scale = nullptr;
};

extern "C" int dspsr_amd_fits_digitizer_create(dspsr_amd_ctx* ctx, uint32_t nchan, uint32_t npol, int nbit, uint32_t nsblk, uint32_t nblock,
                                               int constant, int flip_band, int swap_band, dspsr_amd_fits_digitizer** out)
{
  if (!ctx || !out) return DSPSR_AMD_EINVAL;
  if (nbit != 1 && nbit != 2 && nbit != 4 && nbit != 8)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dsp::FITSDigitizer::set_nbit nbit=%i not understood", nbit);              // :85-86
  if (!nchan || (npol != 1 && npol != 2 && npol != 4))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_create: nchan=%u npol=%u (nchan >= 1, npol 1 / 2 / 4)", nchan, npol);
  if (nchan % (8 / nbit))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_create: nchan=%u not a multiple of %d samples per byte (a byte would "
                    "straddle two polarisations)", nchan, 8 / nbit);
  if (!nsblk) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_create: nsblk == 0");
  if (nsblk > (1u << 30))                                             // (32-bit sample counters in the kernels)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_create: nsblk=%u exceeds 2^30 samples per block", nsblk);
  if (!nblock) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_create: nblock == 0 (at least one block)");
  if ((uint64_t)nchan * npol > 65535)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_create: nchan*npol=%llu exceeds the grid limit",
                    (unsigned long long)nchan * npol);
  dspsr_amd_fits_digitizer* d = new dspsr_amd_fits_digitizer;
  d->ctx = ctx;
  d->nchan = nchan; d->npol = npol; d->ncol = nchan * npol;
  d->nbit = (uint32_t)nbit; d->nsblk = nsblk; d->nblock = nblock;
  d->nslice = (uint32_t)(((uint64_t)nsblk + FITS_SLICE - 1) / FITS_SLICE);
  d->constant = constant != 0;
  d->flip_band = flip_band != 0; d->swap_band = swap_band != 0;
  const float digi_sigma = 8;                                         // set_digi_scales, :14-45
  d->digi_mean = nbit == 1 ? 0.5f : nbit == 2 ? 1.5f : nbit == 4 ? 7.5f : 127.5f;
  d->digi_scale = nbit <= 2 ? 1.f : d->digi_mean / digi_sigma;
  d->digi_max = (1 << nbit) - 1;
  const size_t nd = (size_t)d->ncol * sizeof(double), nf = (size_t)d->ncol * sizeof(float);
  if (hipMalloc((void**)&d->ring_sum, nd * nblock) != hipSuccess || hipMalloc((void**)&d->ring_sq, nd * nblock) != hipSuccess ||
      hipMalloc((void**)&d->offset, nd) != hipSuccess || hipMalloc((void**)&d->scale, nd) != hipSuccess ||
      hipMalloc((void**)&d->part_sum, nd * d->nslice) != hipSuccess || hipMalloc((void**)&d->part_sq, nd * d->nslice) != hipSuccess ||
      hipMalloc((void**)&d->m_offset, nf) != hipSuccess || hipMalloc((void**)&d->m_scale, nf) != hipSuccess) {
    dspsr_amd_fits_digitizer_destroy(d);
    return ctx_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_fits_digitizer_create: hipMalloc failed");
  }
  *out = d;
  return DSPSR_AMD_OK;
}

extern "C" void dspsr_amd_fits_digitizer_destroy(dspsr_amd_fits_digitizer* d)
{
  if (!d) return;
  (void)hipStreamSynchronize(d->ctx->stream);
  double* dbl[] = {d->ring_sum, d->ring_sq, d->offset, d->scale, d->part_sum, d->part_sq};
  for (double* p : dbl) if (p) (void)hipFree(p);
  if (d->m_offset) (void)hipFree(d->m_offset);
  if (d->m_scale) (void)hipFree(d->m_scale);
  delete d;
}

extern "C" int dspsr_amd_fits_digitizer_pack(dspsr_amd_fits_digitizer* d, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                                             void* out_bytes_dev, float* dat_scl_dev, float* dat_offs_dev)
{
  if (!d) return DSPSR_AMD_EINVAL;
  dspsr_amd_ctx* ctx = d->ctx;
  if (!in_dev || !out_bytes_dev || !dat_scl_dev || !dat_offs_dev)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_pack: null pointer (rows, bytes, DAT_SCL and DAT_OFFS are all needed)");
  if ((uintptr_t)in_dev % sizeof(float) || (uintptr_t)dat_scl_dev % sizeof(float) || (uintptr_t)dat_offs_dev % sizeof(float))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_pack: rows and scales must be float aligned");
  const uint32_t n = d->nsblk, nchan = d->nchan, npol = d->npol, ncol = d->ncol;
  if ((npol > 1 && in_pol_stride < n) || (nchan > 1 && in_chan_stride < (uint64_t)(npol - 1) * in_pol_stride + n))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fits_digitizer_pack: input rows of %u floats overlap (chan stride %llu, pol stride %llu)",
                    n, (unsigned long long)in_chan_stride, (unsigned long long)in_pol_stride);
  // measure_scale's walk through its regimes (:181-320), host integers only
  int regime = FITS_KEEP;
  uint32_t idx = 0, old_idx = 0, nrow = 0;
  double recip = 0.0;
  uint32_t next_idx = d->rescale_idx, next_counter = d->rescale_counter;
  if (!(d->constant && d->rescale_counter > 0)) {
    idx = d->rescale_idx == d->nblock ? 0 : d->rescale_idx;           // :188
    if (d->nblock == 1) {
      regime = FITS_SINGLE;
      next_idx = idx; next_counter = 1;
      recip = 1. / n;
    } else if (d->rescale_counter < d->nblock) {
      regime = FITS_FILLING;
      next_counter = nrow = d->rescale_counter + 1;
      recip = (1. / n) * (1. / nrow);
      next_idx = idx + 1;
    } else {
      regime = FITS_FULL;
      old_idx = idx + 1 == d->nblock ? 0 : idx + 1;                   // :308-309 (not the row just overwritten: see DESIGN)
      recip = (1. / n) * (1. / d->nblock);
      next_idx = idx + 1;
    }
    hipLaunchKernelGGL(k_fits_sums, dim3(d->nslice, ncol), dim3(256), 0, ctx->stream, in_dev, in_chan_stride, in_pol_stride, nchan, npol, n,
                       d->part_sum, d->part_sq);
  }
  hipLaunchKernelGGL(k_fits_update, dim3((ncol + 255) / 256), dim3(256), 0, ctx->stream, d->part_sum, d->part_sq, d->nslice, nchan, npol, regime,
                     idx, old_idx, nrow, recip, d->ring_sum, d->ring_sq, d->offset, d->scale, d->m_offset, d->m_scale, d->digi_scale,
                     d->flip_band, d->swap_band, dat_scl_dev, dat_offs_dev);
  const uint32_t ty = (n + 63) / 64;
  hipLaunchKernelGGL(k_fits_pack, dim3((nchan + 63) / 64, ty > 65535 ? 65535 : ty, npol), dim3(256), 0, ctx->stream, in_dev, in_chan_stride,
                     in_pol_stride, (uint8_t*)out_bytes_dev, n, nchan, npol, d->nbit, d->m_offset, d->m_scale, d->digi_scale, d->digi_mean,
                     d->digi_max, d->flip_band, d->swap_band);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_fits_digitizer_pack: %s", hipGetErrorString(e));
  d->rescale_idx = next_idx;                                          // (only once the launches are in)
  d->rescale_counter = next_counter;
  return DSPSR_AMD_OK;
}
