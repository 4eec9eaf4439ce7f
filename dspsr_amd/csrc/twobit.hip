// Two-bit voltages -> float rows with dynamic level setting and excision: dsp::TwoBitCorrection on the device
// (TwoBitCorrection.C:120-150, excision_unpack.h:54-100, TwoBitFour.h:42-89, TwoBitTable.C:42-70).
//
// One input channel of real samples from npol digitisers.  Byte k of the stream belongs to digitiser k % npol and holds four
// consecutive samples of it, the first in the two most significant bits.  A window is nsample samples of one digitiser, nsample / 4
// of its bytes; windows are aligned to the stream, and the block starts with the window that holds the call's first sample
// (`first` inside it).  Both kernels read aligned 32-bit words of the block (little endian: byte k of the stream is bits
// 8 (k & 3) ... of word k >> 2) and work on all sixteen 2-bit fields of a word at once:
//     d  = (v ^ (v >> 1)) & 0x55555555         one bit per field, set where its two bits differ
//     hi = offset binary ~d, sign-magnitude v (the magnitude bit), two's complement d             (& 0x55555555)
//     negative = the sign bit, inverted for offset binary
// and a field is low where it is not hi.
//
// k_twobit_levels: one wave per window, both digitisers of it in one walk (their bytes share the words).  Lanes take the words that
// overlap the window's bytes, mask the bytes of the neighbouring windows, and per digitiser (byte masks 0x00ff00ff / 0xff00ff00)
// count the low fields with a popcount and OR the bytes (TwoBitFour::prepare: bad = every byte zero); the wave reduces them and
// writes, per digitiser, n_low, the weight (excision_unpack.h:83-85) and the window's (lo, hi) pair: entry clamp(n_low, nlow_min,
// nlow_max) - nlow_min of the level table, or (0, 0) for an excised window.
// k_twobit_unpack: one word per lane and step: 16 / npol consecutive samples of each digitiser, each byte with the pair of its own
// window, written with float4 stores where the row address allows, else float2, else by sample; samples outside [0, ndat) of
// the call are not written.
#include "engine_internal.h"

namespace dspsr_amd {

constexpr uint32_t F = 0x55555555u;

// the word at index wi of a block of nbyte bytes; the bytes behind the block's end (a last, partial word) read as zero
__device__ __forceinline__ uint32_t block_word(const uint8_t* __restrict__ raw, const uint64_t wi, const uint64_t nbyte)
{
  if (4 * wi + 4 <= nbyte) return ((const uint32_t*)raw)[wi];
  uint32_t v = 0;
  for (uint64_t k = 4 * wi; k < nbyte; k++) v |= (uint32_t)raw[k] << (8 * (k & 3));
  return v;
}

// one bit per 2-bit field (at the field's low bit): set where the field is a high-voltage state
__device__ __forceinline__ uint32_t hi_fields(const uint32_t v, const int type)
{
  const uint32_t d = (v ^ (v >> 1)) & F;
  return type == DSPSR_AMD_TWOBIT_SIGN_MAGNITUDE ? (v & F) : type == DSPSR_AMD_TWOBIT_OFFSET_BINARY ? (~d & F) : d;
}

__global__ __launch_bounds__(256) void k_twobit_levels(const uint8_t* __restrict__ raw, const uint64_t nbyte, const int type,
                                                       const uint32_t npol, const uint32_t nsample, const uint32_t nwindow,
                                                       const uint32_t nlow_min, const uint32_t nlow_max,
                                                       const float2* __restrict__ levels, float2* __restrict__ pairs,
                                                       uint32_t* __restrict__ weights, uint32_t* __restrict__ nlow_out)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t span = (uint64_t)(nsample / 4) * npol;            // bytes of one window of all digitisers
  // bytes of a digitiser inside a word: every byte, or bytes 0, 2 / 1, 3 (a word starts at an even byte)
  const uint32_t mine0 = npol == 1 ? 0xffffffffu : 0x00ff00ffu, mine1 = ~mine0;
  for (uint32_t win = blockIdx.x * 4 + (threadIdx.x >> 6); win < nwindow; win += gridDim.x * 4) {
    const uint64_t b0 = (uint64_t)win * span, b1 = b0 + span;
    uint32_t count0 = 0, count1 = 0, any0 = 0, any1 = 0;
    for (uint64_t wi = b0 / 4 + lane; 4 * wi < b1; wi += 64) {
      uint32_t m = 0xffffffffu;
      if (4 * wi < b0) m &= 0xffffffffu << (8 * (uint32_t)(b0 - 4 * wi));
      if (4 * wi + 4 > b1) m &= 0xffffffffu >> (8 * (uint32_t)(4 * wi + 4 - b1));
      const uint32_t v = block_word(raw, wi, nbyte) & m;
      const uint32_t low = ~hi_fields(v, type) & F & m;
      count0 += __popc(low & mine0);
      count1 += __popc(low & mine1);
      any0 |= v & mine0;
      any1 |= v & mine1;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      count0 += __shfl_xor(count0, s, 64);
      count1 += __shfl_xor(count1, s, 64);
      any0 |= __shfl_xor(any0, s, 64);
      any1 |= __shfl_xor(any1, s, 64);
    }
    if (lane < npol) {                                             // lane d writes digitiser d
      const uint32_t count = lane ? count1 : count0, any = lane ? any1 : any0, item = lane * nwindow + win;
      const bool bad = any == 0 || count < nlow_min || count > nlow_max;
      const uint32_t use = count < nlow_min ? nlow_min : count > nlow_max ? nlow_max : count;
      const float2 p = levels[use - nlow_min];
      pairs[item] = bad ? make_float2(0.f, 0.f) : p;
      weights[item] = bad ? 0u : 1u;
      if (nlow_out) nlow_out[item] = count;
    }
  }
}

// the four samples of byte `j` of word v, with the window's pair
__device__ __forceinline__ void byte_values(const uint32_t hi, const uint32_t neg, const int j, const float2 pair, float* __restrict__ f)
{
  const uint32_t keep = pair.x != 0.f ? 0x80000000u : 0u;          // an excised window is +0, whatever the sign bit says
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int pos = 8 * j + 6 - 2 * p;
    const float mag = ((hi >> pos) & 1u) ? pair.y : pair.x;
    f[p] = __uint_as_float(__float_as_uint(mag) ^ ((neg << (31 - pos)) & keep));
  }
}

template <int NPOL>
__global__ __launch_bounds__(256) void k_twobit_unpack(const uint8_t* __restrict__ raw, const uint64_t nbyte, const int type,
                                                       const uint32_t nsample, const uint32_t nwindow, const uint32_t first,
                                                       const uint64_t ndat, const float2* __restrict__ pairs,
                                                       float* __restrict__ out, const uint64_t ops)
{
  constexpr int N = 16 / NPOL;                                     // samples of one digitiser in a word
  const uint64_t nword = (nbyte + 3) / 4;
  for (uint64_t wi = (uint64_t)blockIdx.x * 256 + threadIdx.x; wi < nword; wi += (uint64_t)gridDim.x * 256) {
    const uint32_t v = block_word(raw, wi, nbyte);
    const uint32_t hi = hi_fields(v, type);
    const uint32_t neg = ((type == DSPSR_AMD_TWOBIT_OFFSET_BINARY ? ~v : v) >> 1) & F;
    const uint64_t s0 = wi * N;                                    // block sample of the word's first byte of each digitiser
    uint32_t win = (uint32_t)(s0 / nsample), rem = (uint32_t)(s0 - (uint64_t)win * nsample);
    float f[NPOL][N];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int dig = j % NPOL, b = j / NPOL;                      // byte b of the digitiser's share of the word
      const uint32_t w = win < nwindow ? win : nwindow - 1;        // (the zero bytes behind the block's end: never stored)
      byte_values(hi, neg, j, pairs[(uint32_t)dig * nwindow + w], &f[dig][4 * b]);
      if (dig == NPOL - 1) {
        rem += 4;
        if (rem >= nsample) { rem -= nsample; win++; }
      }
    }
    const int64_t n0 = (int64_t)s0 - (int64_t)first;               // sample of the call (negative in front of it)
    const bool whole = n0 >= 0 && (uint64_t)n0 + N <= ndat;
#pragma unroll
    for (int dig = 0; dig < NPOL; dig++) {
      float* __restrict__ row = out + (uint64_t)dig * ops;
      float* __restrict__ o = row + n0;                            // (only formed into addresses of samples inside the row)
      if (whole && ((uintptr_t)o % 16) == 0) {
#pragma unroll
        for (int k = 0; k < N / 4; k++) ((float4*)o)[k] = make_float4(f[dig][4 * k], f[dig][4 * k + 1], f[dig][4 * k + 2], f[dig][4 * k + 3]);
      } else if (whole && ((uintptr_t)o % 8) == 0) {
#pragma unroll
        for (int k = 0; k < N / 2; k++) ((float2*)o)[k] = make_float2(f[dig][2 * k], f[dig][2 * k + 1]);
      } else {
#pragma unroll
        for (int k = 0; k < N; k++) {
          const int64_t n = n0 + k;
          if (n >= 0 && (uint64_t)n < ndat) row[n] = f[dig][k];
        }
      }
    }
  }
}

}  // namespace dspsr_amd

using namespace dspsr_amd;

extern "C" int dspsr_amd_twobit_check(uint64_t raw_addr, int table_type, uint32_t npol, uint32_t nsample, uint32_t first_sample,
                                      uint64_t ndat, uint32_t nlow_min, uint32_t nlow_max, uint64_t out_addr, uint64_t out_pol_stride,
                                      char* msg, size_t msg_len)
{
  const char* who = "dspsr_amd_twobit_unpack";
  if (table_type != DSPSR_AMD_TWOBIT_OFFSET_BINARY && table_type != DSPSR_AMD_TWOBIT_SIGN_MAGNITUDE &&
      table_type != DSPSR_AMD_TWOBIT_TWOS_COMPLEMENT)
    return msg_fail(msg, msg_len, "%s: unknown table_type %d (DSPSR_AMD_TWOBIT_OFFSET_BINARY, _SIGN_MAGNITUDE, _TWOS_COMPLEMENT)", who,
                    table_type);
  if (npol != 1 && npol != 2) return msg_fail(msg, msg_len, "%s: npol=%u not 1 or 2", who, npol);
  if (nsample < 4 || nsample > 65536 || (nsample % 4) != 0)
    return msg_fail(msg, msg_len, "%s: nsample=%u must be a multiple of 4 in [4, 65536] (whole bytes per window)", who, nsample);
  if (nlow_max <= nlow_min || nlow_max > nsample)
    return msg_fail(msg, msg_len, "%s: nlow_min=%u < nlow_max=%u <= nsample=%u must hold", who, nlow_min, nlow_max, nsample);
  if (first_sample >= nsample)
    return msg_fail(msg, msg_len, "%s: first_sample=%u is not inside a window of nsample=%u", who, first_sample, nsample);
  if (ndat >= (1ull << 32) - 65536) return msg_fail(msg, msg_len, "%s: ndat=%llu is too large (< 2^32 - 65536)", who, (unsigned long long)ndat);
  if (raw_addr % 4) return msg_fail(msg, msg_len, "%s: a two-bit block must start at a multiple of 4 bytes (address %#llx)", who,
                                    (unsigned long long)raw_addr);
  if (out_addr % 4) return msg_fail(msg, msg_len, "%s: output rows must be 4-byte aligned (address %#llx)", who,
                                    (unsigned long long)out_addr);
  if (npol > 1 && out_pol_stride < ndat)
    return msg_fail(msg, msg_len, "%s: output rows of %llu floats overlap (pol stride %llu)", who, (unsigned long long)ndat,
                    (unsigned long long)out_pol_stride);
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_twobit_unpack(dspsr_amd_ctx* ctx, const uint8_t* raw_dev, int table_type, uint32_t npol, uint32_t nsample,
                                       uint32_t first_sample, uint64_t ndat, uint32_t nlow_min, uint32_t nlow_max,
                                       const float* levels_dev, float* out_dev, uint64_t out_pol_stride, uint32_t* weights_dev,
                                       uint32_t* nlow_dev)
{
  if (!ctx) return DSPSR_AMD_EINVAL;
  char msg[400];
  const int rc = dspsr_amd_twobit_check((uint64_t)(uintptr_t)raw_dev, table_type, npol, nsample, first_sample, ndat, nlow_min, nlow_max,
                                        (uint64_t)(uintptr_t)out_dev, out_pol_stride, msg, sizeof msg);
  if (rc != DSPSR_AMD_OK) return ctx_fail(ctx, rc, "%s", msg);
  if (!ndat) return DSPSR_AMD_OK;
  if (!raw_dev || !out_dev || !levels_dev || !weights_dev)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_twobit_unpack: null block, level table, output rows or weights");
  const uint32_t nwindow = (uint32_t)((first_sample + ndat + nsample - 1) / nsample), nitem = npol * nwindow;
  const uint64_t nbyte = (uint64_t)nwindow * (nsample / 4) * npol;
  if (!grow_device_buffer(ctx->stream, ctx->window_levels, ctx->window_levels_count, (size_t)nitem))
    return ctx_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_twobit_unpack: hipMalloc(%u level pairs) failed", nitem);
  const uint64_t cap = (uint64_t)(ctx->ncu ? ctx->ncu : 256) * 32;
  const uint64_t nb_levels = ((uint64_t)nwindow + 3) / 4, nb_unpack = ((nbyte + 3) / 4 + 255) / 256;
  hipLaunchKernelGGL(k_twobit_levels, dim3((uint32_t)(nb_levels < cap ? nb_levels : cap)), dim3(256), 0, ctx->stream, raw_dev, nbyte,
                     table_type, npol, nsample, nwindow, nlow_min, nlow_max, (const float2*)levels_dev, ctx->window_levels, weights_dev,
                     nlow_dev);
  const dim3 grid((uint32_t)(nb_unpack < cap ? nb_unpack : cap));
  if (npol == 1)
    hipLaunchKernelGGL(k_twobit_unpack<1>, grid, dim3(256), 0, ctx->stream, raw_dev, nbyte, table_type, nsample, nwindow, first_sample,
                       ndat, (const float2*)ctx->window_levels, out_dev, out_pol_stride);
  else
    hipLaunchKernelGGL(k_twobit_unpack<2>, grid, dim3(256), 0, ctx->stream, raw_dev, nbyte, table_type, nsample, nwindow, first_sample,
                       ndat, (const float2*)ctx->window_levels, out_dev, out_pol_stride);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_twobit_unpack: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
