// GUPPI / PUPPI raw blocks -> float FPT rows (guppi/GUPPIBlockFile.C:214-234 un-transposes every block on the host, one 4-byte
// memcpy per (sample, channel), and guppi/GUPPIUnpacker.C:74-80 then walks the TFP bytes; here the file's bytes stay as they are).
//
// A block's data section is channel-major: run c of block b starts at byte b * block_stride + c * chan_stride and holds the
// consecutive samples of channel c, 2 * npol bytes each: (re, im) of polarisation 0, then of polarisation 1, int8.  Only the first
// block_nsamp samples of a run are kept (the OVERLAP samples behind them repeat the next block's first ones).  With u = first + t,
//     byte of stream sample t = (u / block_nsamp) * block_stride + c * chan_stride + ((u % block_nsamp) * npol + p) * 2 + d,
//     value float(int8): no half step and no scale, unlike every other 8-bit reader of the library.
//
// k_unpack_guppi (one body per npol): a lane takes a group of 16 bytes = 16 / (2 NPOL) samples and writes 32 bytes to each polarisation's row
// (64 to the one row of NPOL 1); the 64 lanes of a wave take consecutive groups of one run: 1 KiB read, 2 KiB stored contiguously
// per row.  The stores are four bytes for every byte read, so the groups are aligned to the OUTPUT: group j holds stream samples
// j G ... j G + G - 1, whose floats start on a 16-byte boundary wherever the row does (float4 stores; else float2, else scalar).
// The run's address decides the load, once per run: a 16-byte load where the group's bytes are 16-byte aligned, else four 32-bit
// loads, else (NPOL 1 at an address that is only even) eight 16-bit loads.  The groups at the two ends of a run's part of the call
// are taken sample by sample, so that no byte outside the kept samples is read and no float outside [0, ndat) is written.
// grid.y walks the (block, channel) runs, grid.x the groups of a run.
#include "fb_common.h"

namespace dspsr_amd {

__device__ __forceinline__ float cvt_i8(uint32_t w, int byte) { return (float)(int8_t)((w >> (8 * byte)) & 0xffu); }

template <int NPOL>
__device__ __forceinline__ void unpack_guppi_runs(const uint8_t* __restrict__ raw, const uint32_t nchan, const uint32_t bn, const uint32_t first,
                                                  const uint64_t cs, const uint64_t bs, const uint64_t ndat, float* __restrict__ out,
                                                  const uint64_t ocs, const uint64_t ops, const uint64_t nrun)
{
  constexpr uint32_t SB = 2 * NPOL, G = 16 / SB, NF = 2 * G;          // bytes per sample; samples per group; floats per row and group
  for (uint64_t run = blockIdx.y; run < nrun; run += gridDim.y) {
    const uint64_t b = run / nchan;
    const uint32_t c = (uint32_t)(run - b * nchan);
    // the run's samples inside the call: stream samples [t_lo, t_hi); sample s of the run is stream sample s + off
    const int64_t off = (int64_t)(b * bn) - (int64_t)first;
    const uint64_t t_lo = b ? (uint64_t)off : 0, t_end = (uint64_t)(off + (int64_t)bn), t_hi = t_end < ndat ? t_end : ndat;
    const uint8_t* __restrict__ src = raw + b * bs + (uint64_t)c * cs;   // (global pointers throughout: no flat loads)
    float* __restrict__ row = out + (uint64_t)c * ocs;
    const uint64_t j_hi = (t_hi + G - 1) / G;
    for (uint64_t j = t_lo / G + (uint64_t)blockIdx.x * 256 + threadIdx.x; j < j_hi; j += (uint64_t)gridDim.x * 256) {
      const uint64_t t0 = j * G;
      if (t0 >= t_lo && t0 + G <= t_hi) {
        const uint8_t* __restrict__ a = src + (uint64_t)((int64_t)t0 - off) * SB;
        uint32_t w[4];
        if (((uintptr_t)a % 16) == 0) {
          const uint4 v = *(const uint4*)a;
          w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else if (NPOL == 2 || ((uintptr_t)a % 4) == 0) {
#pragma unroll
          for (int k = 0; k < 4; k++) w[k] = ((const uint32_t*)a)[k];
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++) w[k] = (uint32_t)((const uint16_t*)a)[2 * k] | ((uint32_t)((const uint16_t*)a)[2 * k + 1] << 16);
        }
#pragma unroll
        for (int p = 0; p < NPOL; p++) {
          float f[NF];
          if (NPOL == 2) {                                  // word s = sample s: bytes 0, 1 polarisation 0, bytes 2, 3 polarisation 1
#pragma unroll
            for (int s = 0; s < 4; s++) { f[2 * s] = cvt_i8(w[s], 2 * p); f[2 * s + 1] = cvt_i8(w[s], 2 * p + 1); }
          } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
              for (int d = 0; d < 4; d++) f[4 * k + d] = cvt_i8(w[k], d);
          }
          float* __restrict__ o = row + (uint64_t)p * ops + 2 * t0;
          if (((uintptr_t)o % 16) == 0) {
#pragma unroll
            for (int k = 0; k < (int)NF / 4; k++) ((float4*)o)[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
          } else if (((uintptr_t)o % 8) == 0) {
#pragma unroll
            for (int k = 0; k < (int)NF / 2; k++) ((float2*)o)[k] = make_float2(f[2 * k], f[2 * k + 1]);
          } else {
#pragma unroll
            for (int k = 0; k < (int)NF; k++) o[k] = f[k];
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < (int)G; k++) {
          const uint64_t t = t0 + k;
          if (t < t_lo || t >= t_hi) continue;
          const uint8_t* __restrict__ a = src + (uint64_t)((int64_t)t - off) * SB;
          const uint32_t w = NPOL == 2 ? *(const uint32_t*)a : (uint32_t)*(const uint16_t*)a;
#pragma unroll
          for (int p = 0; p < NPOL; p++) {
            float* __restrict__ o = row + (uint64_t)p * ops + 2 * t;
            const float re = cvt_i8(w, 2 * p), im = cvt_i8(w, 2 * p + 1);
            if (((uintptr_t)o % 8) == 0) *(float2*)o = make_float2(re, im);
            else { o[0] = re; o[1] = im; }
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_unpack_guppi(const uint8_t* __restrict__ raw, const uint32_t nchan, const uint32_t npol, const uint32_t bn,
                                                      const uint32_t first, const uint64_t cs, const uint64_t bs, const uint64_t ndat,
                                                      float* __restrict__ out, const uint64_t ocs, const uint64_t ops, const uint64_t nrun)
{
  if (npol == 2) unpack_guppi_runs<2>(raw, nchan, bn, first, cs, bs, ndat, out, ocs, ops, nrun);
  else unpack_guppi_runs<1>(raw, nchan, bn, first, cs, bs, ndat, out, ocs, ops, nrun);
}

}  // namespace dspsr_amd

using namespace dspsr_amd;

extern "C" int dspsr_amd_unpack_guppi_fpt(dspsr_amd_ctx* ctx, const int8_t* raw_dev, const dspsr_amd_guppi_layout* lay, uint64_t ndat,
                                          float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride)
{
  if (!ctx) return DSPSR_AMD_EINVAL;
  if (!lay) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: layout is null");
  const uint32_t nchan = lay->nchan, npol = lay->npol, bn = lay->block_nsamp;
  if (!nchan) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: nchan=0 (nchan >= 1)");
  if (npol != 1 && npol != 2) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: npol=%u (npol 1 / 2)", npol);
  if (!bn) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: block_nsamp=0 (a run keeps at least one sample)");
  if (lay->first >= bn)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: first=%u is not inside a block of block_nsamp=%u samples", lay->first, bn);
  const uint64_t sb = 2 * npol, kept = (uint64_t)bn * sb;
  if (lay->chan_stride < kept)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: chan_stride=%llu is shorter than the %llu bytes a run keeps "
                    "(block_nsamp * 2 * npol)", (unsigned long long)lay->chan_stride, (unsigned long long)kept);
  if (nchan > 1 && (lay->chan_stride > (~0ull - kept) / (nchan - 1) || lay->block_stride < (uint64_t)(nchan - 1) * lay->chan_stride + kept))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: block_stride=%llu is shorter than the runs of a block "
                    "((nchan - 1) * chan_stride + block_nsamp * 2 * npol)", (unsigned long long)lay->block_stride);
  if (lay->chan_stride % sb || lay->block_stride % sb)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: chan_stride=%llu, block_stride=%llu: each a multiple of one sample "
                    "(2 * npol = %llu bytes)", (unsigned long long)lay->chan_stride, (unsigned long long)lay->block_stride, (unsigned long long)sb);
  if (((uintptr_t)raw_dev % sb) != 0)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: raw_dev must be a multiple of one sample (2 * npol = %llu bytes)",
                    (unsigned long long)sb);
  if (ndat >= (1ull << 60)) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: ndat is too large");
  const uint64_t nfloat = 2 * ndat;
  if ((npol > 1 && out_pol_stride < nfloat) || (nchan > 1 && out_chan_stride < (npol - 1) * out_pol_stride + nfloat))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: output rows of %llu floats overlap (chan stride %llu, pol stride %llu)",
                    (unsigned long long)nfloat, (unsigned long long)out_chan_stride, (unsigned long long)out_pol_stride);
  if (!ndat) return DSPSR_AMD_OK;
  if (!raw_dev || !out_dev) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_guppi_fpt: null pointer with ndat > 0");
  const uint64_t nblk = (lay->first + ndat + bn - 1) / bn, nrun = nblk * nchan;
  const uint32_t G = 16 / (uint32_t)sb;
  // groups of a run inside the call: at most block_nsamp / G whole ones and one at each end
  const uint64_t ntile = ((uint64_t)bn / G + 2 + 255) / 256, cap = (uint64_t)(ctx->ncu ? ctx->ncu : 256) * 32;
  const uint64_t gx = ntile < cap ? ntile : cap;
  uint64_t gy = cap / gx ? cap / gx : 1;
  if (gy > nrun) gy = nrun;
  if (gy > 65535) gy = 65535;
  const dim3 grid((uint32_t)gx, (uint32_t)gy);
  hipLaunchKernelGGL(k_unpack_guppi, grid, dim3(256), 0, ctx->stream, (const uint8_t*)raw_dev, nchan, npol, bn, lay->first, lay->chan_stride,
                     lay->block_stride, ndat, out_dev, out_chan_stride, out_pol_stride, nrun);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_unpack_guppi_fpt: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
