// MeerKAT beamformer heaps -> float FPT rows (kat/MeerKATUnpacker.C:137-230; CUDA twin MeerKATUnpackerCUDA.cu).
//
// A block is whole heaps of 256 samples.  Heap h holds, for pol in order and then chan in order, the 256 consecutive complex
// samples of that (chan, pol) as (int8 re, int8 im) pairs: run (h * npol + pol) * nchan + chan is 512 contiguous bytes, and
//     byte of stored sample s of heap h = (((h * npol + pol) * nchan + chan) * 256 + s) * 2 + d,   value (float(int8) + 0.5f) * scale.
// Stream sample t of a row is stored at s = t & 255 of heap t >> 8 (MKBF), or at s = (t & 255) ^ 1 (MKBFRo, sample_swap = 2).
//
// k_unpack_heaps: 32 lanes per run, 16 bytes = 8 samples per lane (the block is 16-byte aligned, so every run is); the swap
// exchanges the two samples of each 32-bit word inside the lane.  A run becomes 2 KiB of its row: 64 contiguous bytes per lane,
// four float4 stores where the row address allows, else float2 or scalar stores.  The call's first sample lies at `first` inside
// heap 0 and its last one anywhere inside the last heap: samples outside [0, ndat) are not written.
#include "fb_common.h"

namespace dspsr_amd {

__global__ __launch_bounds__(256) void k_unpack_heaps(const uint4* __restrict__ raw, const float scale, const uint32_t nchan, const uint32_t npol,
                                                      const uint32_t first, const uint32_t swap, const uint64_t ndat, float* __restrict__ out,
                                                      const uint64_t ocs, const uint64_t ops, const uint64_t nrun)
{
  const uint32_t lane = threadIdx.x & 31;
  for (uint64_t run = (uint64_t)blockIdx.x * 8 + (threadIdx.x >> 5); run < nrun; run += (uint64_t)gridDim.x * 8) {
    const uint64_t hp = run / nchan, heap = hp / npol;
    const uint32_t chan = (uint32_t)(run - hp * nchan), pol = (uint32_t)(hp - heap * npol);
    const uint4 v = raw[run * 32 + lane];
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if (swap) {
#pragma unroll
      for (int k = 0; k < 4; k++) w[k] = (w[k] >> 16) | (w[k] << 16);
    }
    float f[16];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      f[4 * k] = cvt8((int8_t)(w[k] & 0xff), scale);
      f[4 * k + 1] = cvt8((int8_t)((w[k] >> 8) & 0xff), scale);
      f[4 * k + 2] = cvt8((int8_t)((w[k] >> 16) & 0xff), scale);
      f[4 * k + 3] = cvt8((int8_t)(w[k] >> 24), scale);
    }
    // stream sample of the lane's first pair, counted from the call's first sample (negative in front of it)
    const int64_t n0 = (int64_t)(heap * 256 + 8 * lane) - (int64_t)first;
    float* __restrict__ row = out + (uint64_t)chan * ocs + (uint64_t)pol * ops;
    float* __restrict__ o = row + 2 * n0;                                 // (only formed into addresses of samples inside the row)
    const bool whole = n0 >= 0 && (uint64_t)n0 + 8 <= ndat;
    if (whole && ((uintptr_t)o % 16) == 0) {
#pragma unroll
      for (int k = 0; k < 4; k++) ((float4*)o)[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
    } else if (((uintptr_t)row % 8) == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int64_t n = n0 + k;
        if (n >= 0 && (uint64_t)n < ndat) ((float2*)row)[n] = make_float2(f[2 * k], f[2 * k + 1]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int64_t n = n0 + k;
        if (n >= 0 && (uint64_t)n < ndat) { row[2 * n] = f[2 * k]; row[2 * n + 1] = f[2 * k + 1]; }
      }
    }
  }
}

}  // namespace dspsr_amd

using namespace dspsr_amd;

extern "C" int dspsr_amd_unpack_heaps_fpt(dspsr_amd_ctx* ctx, const int8_t* raw_dev, int raw_layout, float scale, uint32_t nchan, uint32_t npol,
                                          uint64_t ndat, float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride)
{
  if (!ctx) return DSPSR_AMD_EINVAL;
  const int layout = raw_layout & 0xff;
  const uint32_t first = (uint32_t)raw_layout >> 8;
  if (raw_layout < 0 || (layout != DSPSR_AMD_RAW_MEERKAT && layout != DSPSR_AMD_RAW_MEERKAT_SWAP))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_heaps_fpt: raw_layout %d is not a heap layout (DSPSR_AMD_RAW_MEERKAT, "
                    "DSPSR_AMD_RAW_MEERKAT_SWAP)", raw_layout);
  if (first > 255)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_heaps_fpt: first_sample=%u is not inside a heap of 256 samples", first);
  if (!nchan || (npol != 1 && npol != 2))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_heaps_fpt: nchan=%u npol=%u (nchan >= 1, npol 1 / 2)", nchan, npol);
  if (!ndat) return DSPSR_AMD_OK;
  if (!raw_dev || !out_dev) return DSPSR_AMD_EINVAL;
  if (((uintptr_t)raw_dev % 16) != 0)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_heaps_fpt: a block of heaps must start at a multiple of 16 bytes");
  if (ndat >= (1ull << 60)) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_heaps_fpt: ndat is too large");
  const uint64_t nfloat = 2 * ndat;
  if ((npol > 1 && out_pol_stride < nfloat) || (nchan > 1 && out_chan_stride < (npol - 1) * out_pol_stride + nfloat))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_heaps_fpt: output rows of %llu floats overlap (chan stride %llu, pol stride %llu)",
                    (unsigned long long)nfloat, (unsigned long long)out_chan_stride, (unsigned long long)out_pol_stride);
  const uint64_t nheap = (first + ndat + 255) / 256, nrun = nheap * npol * nchan;
  const uint64_t nblock = (nrun + 7) / 8, cap = (uint64_t)(ctx->ncu ? ctx->ncu : 256) * 32;
  const dim3 grid((uint32_t)(nblock < cap ? nblock : cap));
  hipLaunchKernelGGL(k_unpack_heaps, grid, dim3(256), 0, ctx->stream, (const uint4*)raw_dev, scale, nchan, npol, first,
                     (uint32_t)(layout == DSPSR_AMD_RAW_MEERKAT_SWAP), ndat, out_dev, out_chan_stride, out_pol_stride, nrun);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_unpack_heaps_fpt: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
