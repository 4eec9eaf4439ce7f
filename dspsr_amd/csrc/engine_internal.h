// Shared internals of the C-ABI implementation (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/dspsr_amd.h"
#include "wgfft.h"

struct dspsr_amd_ctx {
  int device;
  hipStream_t stream;
  bool own_stream;
  dspsr_amd::cf* tw;  // exp(-2*pi*i*j/TWN), j < TWN (built in double on the host)
  uint32_t ncu;       // compute units of the device (queried once, at context creation)
  float2* window_levels = nullptr;   // twobit.hip: the (lo, hi) pair of every (digitiser, window) of a call; only grows
  size_t window_levels_count = 0;
  char error[512];
};

// The dynamic-LDS limit is a per-function, process-wide attribute: it is only ever raised (several objects may share a
// kernel with different tile sizes), once per new maximum, outside the per-block calls.
#include <map>
#include <mutex>
inline hipError_t dspsr_amd_allow_lds(const void* kern, size_t bytes)
{
  static std::mutex mtx;
  static std::map<const void*, size_t> limit;
  std::lock_guard<std::mutex> lock(mtx);
  size_t& cur = limit[kern];
  if (bytes <= cur) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) cur = bytes;
  return e;
}

// A device buffer that only grows: a larger request waits for the stream (launches in flight may still use the old block),
// frees it and allocates `need` elements.  false: the allocation failed and the buffer is empty.
template <typename T>
static inline bool grow_device_buffer(hipStream_t stream, T*& buf, size_t& count, size_t need)
{
  if (need <= count) return true;
  (void)hipStreamSynchronize(stream);
  if (buf) (void)hipFree(buf);
  buf = nullptr;
  count = 0;
  if (hipMalloc((void**)&buf, need * sizeof(T)) != hipSuccess) return false;
  count = need;
  return true;
}

static inline void ctx_set_error_v(dspsr_amd_ctx* ctx, const char* fmt, va_list ap)
{
  if (ctx) vsnprintf(ctx->error, sizeof(ctx->error), fmt, ap);
}

static inline int ctx_fail(dspsr_amd_ctx* ctx, int code, const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  ctx_set_error_v(ctx, fmt, ap);
  va_end(ap);
  return code;
}

// The refusal of a device-free check function (dspsr_amd_*_check_*): the text goes to the caller's buffer.
static inline int msg_fail(char* msg, size_t len, const char* fmt, ...)
{
  if (msg && len) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, len, fmt, ap);
    va_end(ap);
  }
  return DSPSR_AMD_EINVAL;
}

// The host shell of the operators that transform tiles and add the detected bins (plfb.hip, bandpass.hip).
//
// The cut of a call's tiles into SEGMENTS of whole tiles, one workgroup per (segment, input channel): enough workgroups to fill the
// chip, at most `cap` segments (the caller's: what its per-segment arrays may take of SEG_BYTES).  Pure: tiles per segment, segments.
constexpr uint32_t SEG_TARGET_WG = 1024;                  // workgroups wanted per launch
constexpr uint32_t SEG_MAX = 256;
constexpr uint64_t SEG_BYTES = 256ull << 20;              // the per-segment arrays of a launch together take at most this
static inline void segment_cut(const uint32_t ntile, const uint32_t nchan_in, const uint64_t cap, uint32_t& tps, uint32_t& nseg)
{
  nseg = SEG_TARGET_WG / nchan_in;
  if (nseg > SEG_MAX) nseg = SEG_MAX;
  if (nseg > cap) nseg = (uint32_t)cap;
  if (nseg > ntile) nseg = ntile;
  if (nseg < 1) nseg = 1;
  tps = (ntile + nseg - 1) / nseg;
  if (tps < 1) tps = 1;
  nseg = (ntile + tps - 1) / tps;
}

// The device array of sums such an operator owns.  `who` names the C-ABI function in the error text.
struct device_sums {
  float* dev = nullptr;
  uint64_t floats = 0;
};
static inline void sums_release(dspsr_amd_ctx* ctx, device_sums& a)
{
  (void)hipStreamSynchronize(ctx->stream);                  // launches in flight may still add to it
  if (a.dev) (void)hipFree(a.dev);
  a.dev = nullptr;
  a.floats = 0;
}
// another size: the old array is released and the new one is NOT zeroed; on failure the array is empty
static inline int sums_resize(dspsr_amd_ctx* ctx, device_sums& a, const uint64_t need, const char* who)
{
  if (need == a.floats) return DSPSR_AMD_OK;
  sums_release(ctx, a);
  if (hipMalloc((void**)&a.dev, need * sizeof(float)) != hipSuccess) {
    a.dev = nullptr;
    return ctx_fail(ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc(%llu floats) failed", who, (unsigned long long)need);
  }
  a.floats = need;
  return DSPSR_AMD_OK;
}
static inline int sums_zero(dspsr_amd_ctx* ctx, device_sums& a, const char* who)
{
  if (!a.dev) return DSPSR_AMD_OK;
  const hipError_t e = hipMemsetAsync(a.dev, 0, a.floats * sizeof(float), ctx->stream);
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
// copies the sums to the host and waits
static inline int sums_synch(dspsr_amd_ctx* ctx, const device_sums& a, float* host, const char* who)
{
  if (!a.dev) return ctx_fail(ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
  hipError_t e = hipMemcpyAsync(host, a.dev, a.floats * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
