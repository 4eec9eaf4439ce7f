// SIGPROC filterbank spectra -> float FPT rows (dsp::SigProcUnpacker::unpack, OrderFPT branch, sigproc/SigProcUnpacker.C:96-156: one
// host loop per (channel, polarisation) row that walks the file with a stride of one spectrum).
//
// The file is time-major: spectrum t is the S = npol * nchan * nbit / 8 bytes at raw + t * S, value v = ipol * nchan + ichan of it
// belongs to row (ichan, ipol), float t.  nbit 8 / 16 / 32: element v as uint8 / uint16 / a float copied bit for bit; nbit 1 / 2 / 4:
// bits [v * nbit, (v + 1) * nbit) of the spectrum read as a little-endian bit stream (the lowest bits of a byte are the first
// channel).  The value is float(x) - offset, offset = 127.5 (nbit 8) or 32768 (nbit 16) in the rows ipol > 1, else 0: exact in float32.
//
// This is a transpose, so k_unpack_sigproc<NBIT, LW> takes it as tiles through LDS: a workgroup takes T = 64 consecutive spectra by
// V = 128 consecutive values (16 * NBIT bytes of the spectrum).
//   load   a lane takes a unit of LW bytes = U = 8 LW / NBIT values; the UPT = V / U units of a spectrum lie along the lanes, four
//          spectra side by side in the two lowest lane bits (a wave reads runs of 16 LW bytes of four spectra).  LW is the widest
//          load raw and S allow -- 16, 8, 4, 2 or 1 bytes, never more than an eighth of the tile's span -- decided once per call.  Every
//          value of the unit is unpacked from the loaded words in registers.
//   LDS    value j of unit u goes to image row r = j * UPT + u, a row is the 64 floats of the tile's spectra rotated by 4 * (r / 2 % 16)
//          floats.  Write (ds_write_b32, 32 banks, 32-lane halves): the lanes of a half hold 8 consecutive rows by 4 consecutive
//          spectra, 16 banks with two lanes each, which costs nothing.  Read (ds_read_b128, 64 banks, 16-lane groups that pair the
//          rows r, r + 1 with r even): a row's 16 lanes read the 16 float4 of the row, both rows of a group rotated alike: no bank
//          is asked twice.  Rotating by whole float4 keeps every lane's four floats together.
//   store  lanes along time: 16 lanes x float4 = the 256 contiguous bytes of a row, float4 where the row's address in the tile is
//          16-byte aligned, four scalar stores otherwise; the per-row offset is subtracted here.
// A tile that is not whole -- the last values of a spectrum, the last spectra of the call, npol * nchan < 128 -- takes its values
// one by one, lanes along time, without the LDS.  Nothing outside raw ... raw + ndat * S is read, nothing outside the ndat floats of
// a row is written.  Byte model: nbit / 8 bytes read + 4 written per value.
#include "fb_common.h"

namespace dspsr_amd {

constexpr uint32_t SPT = 64, SPV = 128;      // spectra and values per tile

template <int NBIT>
__device__ __forceinline__ float sigproc_row_offset(const uint32_t ipol)
{
  return NBIT == 8 ? (ipol > 1 ? 127.5f : 0.f) : NBIT == 16 ? (ipol > 1 ? 32768.f : 0.f) : 0.f;
}

template <int NBIT, int LW>
__global__ __launch_bounds__(256) void k_unpack_sigproc(const uint8_t* __restrict__ raw, const uint32_t nchan, const uint64_t nval, const uint64_t S,
                                                        const uint64_t ndat, float* __restrict__ out, const uint64_t ocs, const uint64_t ops)
{
  constexpr uint32_t U = 8 * LW / NBIT, UPT = SPV / U, NW = LW < 4 ? 1 : LW / 4, MASK = NBIT == 32 ? 0xffffffffu : (1u << (NBIT & 31)) - 1u;
  static_assert(UPT >= 8 && U >= 1 && U * UPT == SPV, "a unit is at most an eighth of the tile's span");
  __shared__ float img[SPV * SPT];
  const uint32_t tid = threadIdx.x;
  const uint64_t v0 = (uint64_t)blockIdx.x * SPV, byte0 = v0 * NBIT / 8;
  const uint64_t ntile = (ndat + SPT - 1) / SPT;
  FB_ST_BEGIN(9);
  for (uint64_t tile = blockIdx.y; tile < ntile; tile += gridDim.y) {
    const uint64_t t0 = tile * SPT;
    if (v0 + SPV <= nval && t0 + SPT <= ndat) {
      FB_ST(9, 0);                       // (stamped builds: the stores of the tile before have drained)
      const uint8_t* __restrict__ src = raw + t0 * S + byte0;
#pragma unroll 2
      for (uint32_t q = tid; q < SPT * UPT; q += 256) {
        const uint32_t u = (q >> 2) % UPT, t = (q / (4 * UPT)) * 4 + (q & 3);
        const uint8_t* __restrict__ a = src + (uint64_t)t * S + u * LW;
        uint32_t w[NW];
        if constexpr (LW == 16) {
          const uint4 x = *(const uint4*)a;
          w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
        } else if constexpr (LW == 8) {
          const uint2 x = *(const uint2*)a;
          w[0] = x.x; w[1] = x.y;
        } else if constexpr (LW == 4) w[0] = *(const uint32_t*)a;
        else if constexpr (LW == 2) w[0] = *(const uint16_t*)a;
        else w[0] = *a;
#pragma unroll
        for (uint32_t j = 0; j < U; j++) {
          const uint32_t x = (w[(j * NBIT) >> 5] >> ((j * NBIT) & 31)) & MASK;
          const uint32_t r = j * UPT + u;
          img[r * SPT + ((t + 4 * ((r >> 1) & 15)) & (SPT - 1))] = NBIT == 32 ? __uint_as_float(x) : (float)x;
        }
      }
      __syncthreads();
      FB_ST(9, 1);
#pragma unroll 2
      for (uint32_t k = tid; k < SPV * (SPT / 4); k += 256) {
        const uint32_t r = k >> 4, f = k & 15;
        const uint64_t v = v0 + (r % UPT) * U + r / UPT;
        const uint32_t ipol = (uint32_t)(v / nchan), ichan = (uint32_t)(v - (uint64_t)ipol * nchan);
        float4 x = *(const float4*)&img[r * SPT + ((4 * f + 4 * ((r >> 1) & 15)) & (SPT - 1))];
        if (NBIT == 8 || NBIT == 16) {
          const float off = sigproc_row_offset<NBIT>(ipol);
          x.x -= off; x.y -= off; x.z -= off; x.w -= off;
        }
        float* __restrict__ o = out + (uint64_t)ichan * ocs + (uint64_t)ipol * ops + t0 + 4 * f;
        if (((uintptr_t)o % 16) == 0) *(float4*)o = x;
        else { o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w; }
      }
      __syncthreads();
      FB_ST(9, 2);
      FB_ST_TILE(9, 3);
    } else {
      // an edge tile: value by value, lanes along time
      const uint64_t nv = nval - v0 < SPV ? nval - v0 : SPV, nt = ndat - t0 < SPT ? ndat - t0 : SPT;
      for (uint64_t k = tid; k < nv * SPT; k += 256) {
        const uint64_t t = k & (SPT - 1), v = v0 + (k >> 6);
        if (t >= nt) continue;
        const uint8_t* __restrict__ a = raw + (t0 + t) * S;
        const uint32_t ipol = (uint32_t)(v / nchan), ichan = (uint32_t)(v - (uint64_t)ipol * nchan);
        float x;
        if (NBIT == 32) x = __uint_as_float(((const uint32_t*)a)[v]);
        else if (NBIT == 16) x = (float)((const uint16_t*)a)[v] - sigproc_row_offset<NBIT>(ipol);
        else x = (float)(((uint32_t)a[v * NBIT / 8] >> ((v * NBIT) & 7)) & MASK) - sigproc_row_offset<NBIT>(ipol);
        out[(uint64_t)ichan * ocs + (uint64_t)ipol * ops + t0 + t] = x;
      }
    }
  }
  FB_ST_END(9);
}

template <int NBIT, int LW>
static void launch_unpack_sigproc(dspsr_amd_ctx* ctx, const dim3 grid, const uint8_t* raw, uint32_t nchan, uint64_t nval, uint64_t S, uint64_t ndat,
                                  float* out, uint64_t ocs, uint64_t ops)
{
  hipLaunchKernelGGL((k_unpack_sigproc<NBIT, LW>), grid, dim3(256), 0, ctx->stream, raw, nchan, nval, S, ndat, out, ocs, ops);
}

// the widest load of the tile for this call: LW divides the address of every unit (raw, S; a tile starts on a multiple of 16 bytes)
template <int NBIT>
static void dispatch_unpack_sigproc(dspsr_amd_ctx* ctx, const dim3 grid, const uint8_t* raw, uint32_t nchan, uint64_t nval, uint64_t S, uint64_t ndat,
                                    float* out, uint64_t ocs, uint64_t ops)
{
  const uint64_t a = (uint64_t)(uintptr_t)raw | S;
  constexpr int MAXLW = 2 * NBIT < 16 ? 2 * NBIT : 16;      // an eighth of the tile's 16 * NBIT bytes
  if constexpr (MAXLW >= 16) if (a % 16 == 0) return launch_unpack_sigproc<NBIT, 16>(ctx, grid, raw, nchan, nval, S, ndat, out, ocs, ops);
  if constexpr (MAXLW >= 8) if (a % 8 == 0) return launch_unpack_sigproc<NBIT, 8>(ctx, grid, raw, nchan, nval, S, ndat, out, ocs, ops);
  if constexpr (MAXLW >= 4) if (a % 4 == 0) return launch_unpack_sigproc<NBIT, 4>(ctx, grid, raw, nchan, nval, S, ndat, out, ocs, ops);
  if constexpr (NBIT <= 16) if (a % 2 == 0) return launch_unpack_sigproc<NBIT, 2>(ctx, grid, raw, nchan, nval, S, ndat, out, ocs, ops);
  if constexpr (NBIT <= 8) launch_unpack_sigproc<NBIT, 1>(ctx, grid, raw, nchan, nval, S, ndat, out, ocs, ops);
}

}  // namespace dspsr_amd

using namespace dspsr_amd;

extern "C" int dspsr_amd_unpack_sigproc_fpt(dspsr_amd_ctx* ctx, const void* raw_dev, uint32_t nbit, uint32_t nchan, uint32_t npol, uint64_t ndat,
                                            float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride)
{
  if (!ctx) return DSPSR_AMD_EINVAL;
  if (nbit != 1 && nbit != 2 && nbit != 4 && nbit != 8 && nbit != 16 && nbit != 32)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_sigproc_fpt: nbit=%u (nbit 1 / 2 / 4 / 8 / 16 / 32)", nbit);
  if (!nchan) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_sigproc_fpt: nchan=0 (nchan >= 1)");
  if (npol != 1 && npol != 2 && npol != 4) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_sigproc_fpt: npol=%u (npol 1 / 2 / 4)", npol);
  if (nbit < 8 && ((uint64_t)nchan * nbit) % 8)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_sigproc_fpt: nchan=%u of %u bits do not fill whole bytes (nchan * nbit a multiple of 8: "
                    "a polarisation starts on a byte)", nchan, nbit);
  if (nbit > 8 && ((uintptr_t)raw_dev % (nbit / 8)) != 0)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_sigproc_fpt: raw_dev must be a multiple of one value (%u bytes)", nbit / 8);
  const uint64_t nval = (uint64_t)npol * nchan, S = nval * nbit / 8;
  if (ndat > (1ull << 62) / S) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_sigproc_fpt: ndat is too large (ndat * spectrum bytes <= 2^62)");
  if ((npol > 1 && out_pol_stride < ndat) || (nchan > 1 && out_chan_stride < (npol - 1) * out_pol_stride + ndat))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_sigproc_fpt: output rows of %llu floats overlap (chan stride %llu, pol stride %llu)",
                    (unsigned long long)ndat, (unsigned long long)out_chan_stride, (unsigned long long)out_pol_stride);
  if (!ndat) return DSPSR_AMD_OK;
  if (!raw_dev || !out_dev) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_sigproc_fpt: null pointer with ndat > 0");
  const uint64_t gx = (nval + SPV - 1) / SPV, ntile = (ndat + SPT - 1) / SPT;
  const dim3 grid((uint32_t)gx, (uint32_t)(ntile < 65535 ? ntile : 65535));
  const uint8_t* raw = (const uint8_t*)raw_dev;
  switch (nbit) {
    case 1: dispatch_unpack_sigproc<1>(ctx, grid, raw, nchan, nval, S, ndat, out_dev, out_chan_stride, out_pol_stride); break;
    case 2: dispatch_unpack_sigproc<2>(ctx, grid, raw, nchan, nval, S, ndat, out_dev, out_chan_stride, out_pol_stride); break;
    case 4: dispatch_unpack_sigproc<4>(ctx, grid, raw, nchan, nval, S, ndat, out_dev, out_chan_stride, out_pol_stride); break;
    case 8: dispatch_unpack_sigproc<8>(ctx, grid, raw, nchan, nval, S, ndat, out_dev, out_chan_stride, out_pol_stride); break;
    case 16: dispatch_unpack_sigproc<16>(ctx, grid, raw, nchan, nval, S, ndat, out_dev, out_chan_stride, out_pol_stride); break;
    default: dispatch_unpack_sigproc<32>(ctx, grid, raw, nchan, nval, S, ndat, out_dev, out_chan_stride, out_pol_stride); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_unpack_sigproc_fpt: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

FB_ST_READER(unpack_sigproc)
