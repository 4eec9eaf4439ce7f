// Phase-locked filterbank (dspsr -G nbin): dsp::PhaseLockedFilterbank on the device.
//
// Semantics: the loop body of Signal/Pulsar/PhaseLockedFilterbank.C:254-297.  A WINDOW is (idat_start, bin): nchan complex
// samples (Analytic rows) or 2 nchan real samples (Nyquist rows) of every input channel and polarisation from idat_start on are
// transformed (forward, unnormalised), square-law detected and added into phase bin `bin` of output channel chan * nchan + k.
//
// The tile -- C = nchan complex points x the (window, polarisation) columns of Tp = 8192 / C windows, its staged transform, the
// Hermitian split of Nyquist rows, detection and the register sums of the bins a thread owns -- is spectral_tile.h's, shared with
// k_bandpass.  Here: the load of a window from the window list, and where the sums go.
//
// Accumulation: the host sorts the call's windows by bin (stable: time order inside a bin) and cuts the sorted list into
// SEGMENTS of whole tiles; workgroup (segment, input channel) walks its windows in order and keeps a bin's sums in registers
// until the bin changes.  A bin whose windows all lie in one segment is added to the profile by that segment (its only owner
// in the launch).  A bin that spans segments is written, per segment, to a SLOT of its own, and k_plfb_combine -- one owner
// per element again -- adds the slots to the profile in segment order.  No atomics; the cut depends on the call's arguments
// alone, so the same sequence of calls gives the same bits.
#include <string.h>

#include <algorithm>
#include <vector>

#include "engine_internal.h"
#include "spectral_tile.h"

namespace dspsr_amd {

constexpr uint32_t PL_SLOT = 0x80000000u;                 // destination flag: a slot, not a bin of the profile

struct PlfbArgs {
  const float* in;                // element (chan, pol, t) = in + chan * cs + pol * ps + t * ndim
  uint64_t cs, ps;
  float* prof;                    // [nchan_out][npol_out][nbin]
  float* slots;                   // [slot][npol_out][nchan_out]
  const uint32_t* wstart;         // sorted windows: first sample
  const uint32_t* wdst;           //                 bin, or PL_SLOT | slot
  uint32_t nwin, wps;             // windows of the call; windows per segment (a multiple of the tile's)
  uint32_t nbin, nchan_out, npol_in;
};

template <int LOGC, int NDIM, int NPO>
__global__ __launch_bounds__(ST_THREADS) void k_plfb(const PlfbArgs a, const cf* __restrict__ tw)
{
  // NPO == 1: p0 + p1, two input polarisations give total intensity; the Nyquist twiddles are always held in registers
  typedef SpectralTile<LOGC, NDIM, NPO, true, 8> T;
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  const uint32_t tid = threadIdx.x;
  const uint32_t ltw_off = T::fill_twiddle_table(lds, tw, tid);
  const uint32_t chan = blockIdx.y, seg = blockIdx.x;
  const uint32_t w_begin = seg * a.wps, w_end = min(w_begin + a.wps, a.nwin);
  const float* const row0 = a.in + chan * a.cs;
  const float* const row1 = row0 + a.ps;
  const bool two = a.npol_in > 1;                           // one input polarisation: the second column of every pair is zero

  typename T::Tw wc, ws;
  T::twiddles(wc, ws);
  typename T::Acc acc;
  T::zero(acc);
  uint32_t cur = 0xffffffffu;                               // destination of the sums held (uniform); none yet

  // adds the sums to their destination -- this workgroup is its only owner in the launch -- and clears them
  auto flush = [&](const uint32_t d) {
    T::for_owned([&](const int j, const int e, const uint32_t bin) {
      const size_t co = (size_t)chan * T::C + bin;
#pragma unroll
      for (int q = 0; q < NPO; q++) {
        if (d & PL_SLOT) {
          a.slots[((size_t)(d & ~PL_SLOT) * NPO + q) * a.nchan_out + co] = acc[j][e][q];
        } else {
          float* const dst = a.prof + (co * NPO + q) * a.nbin + d;
          *dst += acc[j][e][q];
        }
      }
    });
    T::zero(acc);
  };
  // window w starts at sample wstart[w]
  auto load = [&](const uint32_t w, const uint32_t n, float2& v0, float2& v1) {
    const uint32_t s = a.wstart[w];
    if constexpr (NDIM == 2) {
      v0 = reinterpret_cast<const float2*>(row0)[s + n];
      if (two) v1 = reinterpret_cast<const float2*>(row1)[s + n];
    } else {
      const size_t o = (size_t)s + 2 * n;                   // any parity of s: two 4-byte loads
      v0 = make_float2(row0[o], row0[o + 1]);
      if (two) v1 = make_float2(row1[o], row1[o + 1]);
    }
  };

  for (uint32_t w0 = w_begin; w0 < w_end; w0 += T::Tp) {
    uint32_t t = tid;                                       // (a copy: see transform)
    T::transform(lds, ltw_off, t, w0, w_end, load);
    const uint32_t nw = min(T::Tp, w_end - w0);
    for (uint32_t c2 = 0; c2 < nw; c2++) {
      const uint32_t d = __builtin_amdgcn_readfirstlane(a.wdst[w0 + c2]);
      if (d != cur) {
        if (cur != 0xffffffffu) flush(cur);
        cur = d;
      }
      T::add_part(acc, lds, c2, wc, ws);
    }
    __syncthreads();                                        // the next tile's exchanges overwrite the staged image
  }
  if (cur != 0xffffffffu) flush(cur);
}

// profile[bin] += slot0 + slot1 + ... of every bin that spans segments, in segment order; ent = (bin, first slot, slots)
__global__ __launch_bounds__(256) void k_plfb_combine(float* __restrict__ prof, const float* __restrict__ slots,
                                                      const uint32_t* __restrict__ ent, const uint32_t nchan_out,
                                                      const uint32_t npo, const uint32_t nbin)
{
  const uint32_t bin = ent[3 * blockIdx.y], s0 = ent[3 * blockIdx.y + 1], ns = ent[3 * blockIdx.y + 2];
  const size_t n = (size_t)nchan_out * npo;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t q = i / nchan_out, co = i - q * nchan_out;
  float* const dst = prof + (co * npo + q) * nbin + bin;
  float v = *dst;
  for (uint32_t s = 0; s < ns; s++) v += slots[(size_t)(s0 + s) * n + i];
  *dst = v;
}

typedef void (*kplfb_t)(PlfbArgs, const cf*);
template <int NDIM, int NPO> static kplfb_t pick_plfb2(const int logc)
{
  static const kplfb_t t[] = {nullptr, k_plfb<1, NDIM, NPO>, k_plfb<2, NDIM, NPO>, k_plfb<3, NDIM, NPO>, k_plfb<4, NDIM, NPO>,
                              k_plfb<5, NDIM, NPO>, k_plfb<6, NDIM, NPO>, k_plfb<7, NDIM, NPO>, k_plfb<8, NDIM, NPO>,
                              k_plfb<9, NDIM, NPO>, k_plfb<10, NDIM, NPO>, k_plfb<11, NDIM, NPO>, k_plfb<12, NDIM, NPO>,
                              k_plfb<13, NDIM, NPO>};
  return t[logc];
}
static kplfb_t pick_plfb(const int logc, const uint32_t ndim, const uint32_t npo)
{
  if (ndim == 2) return npo == 1 ? pick_plfb2<2, 1>(logc) : npo == 2 ? pick_plfb2<2, 2>(logc) : pick_plfb2<2, 4>(logc);
  return npo == 1 ? pick_plfb2<1, 1>(logc) : npo == 2 ? pick_plfb2<1, 2>(logc) : pick_plfb2<1, 4>(logc);
}

}  // namespace dspsr_amd
using namespace dspsr_amd;

struct dspsr_amd_plfb {
  dspsr_amd_ctx* ctx = nullptr;
  uint32_t nchan_in = 0, npol_in = 0, ndim_in = 0, nchan = 0, npol_out = 0, nbin = 0;
  device_sums prof;                 // [nchan_out][npol_out][nbin]
  float* slots = nullptr;
  size_t slot_count = 0;
  std::vector<uint32_t> order, host;
  uint32_t* dev = nullptr;
  size_t dev_count = 0;
};

extern "C" int dspsr_amd_plfb_check_shape(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t nchan,
                                          uint32_t npol_out, uint32_t nbin, char* msg, size_t msg_len)
{
  const char* who = "dspsr_amd_plfb_set_shape";
  if (nchan < 2 && nbin < 2)                                // PhaseLockedFilterbank.C:61-63
    return msg_fail(msg, msg_len, "%s: invalid dimensions.  nchan=%u nbin=%u", who, nchan, nbin);
  if (!nchan_in || !nbin) return msg_fail(msg, msg_len, "%s: zero dimension (nchan_in=%u nbin=%u)", who, nchan_in, nbin);
  if (nchan < 2 || nchan > 8192 || (nchan & (nchan - 1)))
    return msg_fail(msg, msg_len, "%s: nchan=%u must be a power of two in [2, 8192]", who, nchan);
  if (npol_out != 1 && npol_out != 2 && npol_out != 4)      // :44-46
    return msg_fail(msg, msg_len, "%s: Invalid npol (%u)", who, npol_out);
  if (npol_in != 1 && npol_in != 2) return msg_fail(msg, msg_len, "%s: npol_in=%u not 1 or 2", who, npol_in);
  if (npol_in < 2 && npol_out > 1)                          // :138-141
    return msg_fail(msg, msg_len, "%s: Not enough input polns (%u) for output npol (%u)", who, npol_in, npol_out);
  if (ndim_in != 1 && ndim_in != 2)                         // :102-110
    return msg_fail(msg, msg_len, "%s: ndim_in=%u is neither Nyquist (1) nor Analytic (2)", who, ndim_in);
  if (nchan_in > 65535 || (uint64_t)nchan_in * nchan >= (1ull << 31) || nbin >= (1u << 31))
    return msg_fail(msg, msg_len, "%s: nchan_in=%u > 65535, nchan_in * nchan or nbin=%u >= 2^31", who, nchan_in, nbin);
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_plfb_check_windows(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t nchan, uint32_t nbin,
                                            uint64_t in_addr, uint64_t chan_stride, uint64_t pol_stride, uint64_t ndat,
                                            uint64_t nwin, const uint64_t* idat_start_host, const uint32_t* bin_host, char* msg,
                                            size_t msg_len)
{
  const char* who = "dspsr_amd_plfb_accumulate";
  const uint64_t ndat_fft = ndim_in == 2 ? nchan : 2ull * nchan;            // :100-110
  if (ndat >= (1ull << 31) || nwin >= (1ull << 31))
    return msg_fail(msg, msg_len, "%s: ndat=%llu or nwin=%llu >= 2^31", who, (unsigned long long)ndat, (unsigned long long)nwin);
  if (nwin && (!idat_start_host || !bin_host)) return msg_fail(msg, msg_len, "%s: null window list", who);
  // Analytic rows are read as 8-byte complex samples, Nyquist rows as floats
  if ((in_addr & 3) || (ndim_in == 2 && ((in_addr & 7) || (chan_stride & 1) || (pol_stride & 1))))
    return msg_fail(msg, msg_len, "%s: rows must be %u-byte aligned (address %#llx, strides %llu, %llu floats)", who,
                    ndim_in == 2 ? 8u : 4u, (unsigned long long)in_addr, (unsigned long long)chan_stride,
                    (unsigned long long)pol_stride);
  const uint64_t row = ndat * ndim_in;
  if ((npol_in > 1 && pol_stride < row) || (nchan_in > 1 && chan_stride < row))
    return msg_fail(msg, msg_len, "%s: stride shorter than the row of %llu floats", who, (unsigned long long)row);
  for (uint64_t w = 0; w < nwin; w++) {
    if (idat_start_host[w] + ndat_fft > ndat)
      return msg_fail(msg, msg_len, "%s: window %llu: idat_start=%llu + ndat_fft=%llu > ndat=%llu", who, (unsigned long long)w,
                      (unsigned long long)idat_start_host[w], (unsigned long long)ndat_fft, (unsigned long long)ndat);
    if (bin_host[w] >= nbin)
      return msg_fail(msg, msg_len, "%s: window %llu: bin=%u >= nbin=%u", who, (unsigned long long)w, bin_host[w], nbin);
    if (w && idat_start_host[w] < idat_start_host[w - 1])
      return msg_fail(msg, msg_len, "%s: window %llu: idat_start=%llu before its predecessor's %llu: windows out of time order",
                      who, (unsigned long long)w, (unsigned long long)idat_start_host[w],
                      (unsigned long long)idat_start_host[w - 1]);
  }
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_plfb_create(dspsr_amd_ctx* ctx, dspsr_amd_plfb** out)
{
  if (!ctx || !out) return DSPSR_AMD_EINVAL;
  dspsr_amd_plfb* f = new dspsr_amd_plfb;
  f->ctx = ctx;
  *out = f;
  return DSPSR_AMD_OK;
}

extern "C" void dspsr_amd_plfb_destroy(dspsr_amd_plfb* f)
{
  if (!f) return;
  sums_release(f->ctx, f->prof);
  if (f->slots) (void)hipFree(f->slots);
  if (f->dev) (void)hipFree(f->dev);
  delete f;
}

extern "C" int dspsr_amd_plfb_zero(dspsr_amd_plfb* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  return sums_zero(f->ctx, f->prof, "dspsr_amd_plfb_zero");
}

extern "C" int dspsr_amd_plfb_set_shape(dspsr_amd_plfb* f, uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t nchan,
                                        uint32_t npol_out, uint32_t nbin)
{
  if (!f) return DSPSR_AMD_EINVAL;
  char msg[400];
  const int rc = dspsr_amd_plfb_check_shape(nchan_in, npol_in, ndim_in, nchan, npol_out, nbin, msg, sizeof msg);
  if (rc != DSPSR_AMD_OK) return ctx_fail(f->ctx, rc, "%s", msg);
  const bool changed = nchan_in != f->nchan_in || npol_in != f->npol_in || ndim_in != f->ndim_in || nchan != f->nchan ||
                       npol_out != f->npol_out || nbin != f->nbin;
  if (sums_resize(f->ctx, f->prof, (uint64_t)nchan_in * nchan * npol_out * nbin, "dspsr_amd_plfb_set_shape") != DSPSR_AMD_OK) {
    f->nbin = 0;
    return DSPSR_AMD_ENOMEM;
  }
  f->nchan_in = nchan_in; f->npol_in = npol_in; f->ndim_in = ndim_in; f->nchan = nchan; f->npol_out = npol_out; f->nbin = nbin;
  return changed ? dspsr_amd_plfb_zero(f) : DSPSR_AMD_OK;   // a new shape starts from zero; the same shape keeps its sums
}

extern "C" int dspsr_amd_plfb_accumulate(dspsr_amd_plfb* f, const float* in_dev, uint64_t chan_stride, uint64_t pol_stride,
                                         uint64_t ndat, uint64_t nwin, const uint64_t* idat_start_host, const uint32_t* bin_host)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_plfb_accumulate";
  if (!f->prof.dev) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
  char msg[400];
  const int rc = dspsr_amd_plfb_check_windows(f->nchan_in, f->npol_in, f->ndim_in, f->nchan, f->nbin, (uint64_t)(uintptr_t)in_dev,
                                              chan_stride, pol_stride, ndat, nwin, idat_start_host, bin_host, msg, sizeof msg);
  if (rc != DSPSR_AMD_OK) return ctx_fail(f->ctx, rc, "%s", msg);
  if (!nwin) return DSPSR_AMD_OK;
  if (!in_dev) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: null input", who);

  int logc = 0;
  while ((1u << logc) < f->nchan) logc++;
  const uint32_t tp = 8192u >> logc;                        // windows per tile
  const uint32_t n = (uint32_t)nwin, nchan_out = f->nchan_in * f->nchan;
  // segments within the memory set aside for the slots (two per segment at most)
  const uint64_t slot_floats = (uint64_t)f->npol_out * nchan_out;
  uint32_t tps, nseg;
  segment_cut((n + tp - 1) / tp, f->nchan_in, SEG_BYTES / (2 * slot_floats * sizeof(float)), tps, nseg);
  const uint32_t wps = tps * tp;

  // windows by bin, time order inside a bin
  f->order.resize(n);
  for (uint32_t i = 0; i < n; i++) f->order[i] = i;
  std::stable_sort(f->order.begin(), f->order.end(), [&](const uint32_t x, const uint32_t y) { return bin_host[x] < bin_host[y]; });
  f->host.assign(2 * (size_t)n, 0);
  uint32_t nslot = 0;
  std::vector<uint32_t> ent;
  for (uint32_t lo = 0; lo < n;) {
    const uint32_t bin = bin_host[f->order[lo]];
    uint32_t hi = lo + 1;
    while (hi < n && bin_host[f->order[hi]] == bin) hi++;
    const uint32_t s_lo = lo / wps, s_hi = (hi - 1) / wps;
    if (s_lo != s_hi) {
      ent.push_back(bin); ent.push_back(nslot); ent.push_back(s_hi - s_lo + 1);
    }
    for (uint32_t i = lo; i < hi; i++) {
      f->host[i] = (uint32_t)idat_start_host[f->order[i]];
      f->host[n + i] = s_lo == s_hi ? bin : (PL_SLOT | (nslot + (i / wps - s_lo)));
    }
    if (s_lo != s_hi) nslot += s_hi - s_lo + 1;
    lo = hi;
  }
  const size_t ent_off = f->host.size();
  f->host.insert(f->host.end(), ent.begin(), ent.end());

  hipStream_t s = f->ctx->stream;
  if (!grow_device_buffer(s, f->dev, f->dev_count, f->host.size()))
    return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc(%zu plan entries) failed", who, f->host.size());
  if (nslot && !grow_device_buffer(s, f->slots, f->slot_count, (size_t)nslot * slot_floats))
    return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc(%u slots of %llu floats) failed", who, nslot,
                    (unsigned long long)slot_floats);
  // (the copy reads f->host when it is issued -- pageable memory is staged before the call returns -- and the stream orders it
  //  behind the launches of the previous call that still read the old lists)
  hipError_t err = hipMemcpyAsync(f->dev, f->host.data(), f->host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: plan upload: %s", who, hipGetErrorString(err));

  PlfbArgs a;
  a.in = in_dev; a.cs = chan_stride; a.ps = pol_stride;
  a.prof = f->prof.dev; a.slots = f->slots;
  a.wstart = f->dev; a.wdst = f->dev + n;
  a.nwin = n; a.wps = wps; a.nbin = f->nbin; a.nchan_out = nchan_out; a.npol_in = f->npol_in;
  const kplfb_t k = pick_plfb(logc, f->ndim_in, f->npol_out);
  const size_t lds = lds_total_words_host(16384, logc) * sizeof(cf);
  err = dspsr_amd_allow_lds((const void*)k, lds);
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(err));
  hipLaunchKernelGGL(k, dim3(nseg, f->nchan_in), dim3(ST_THREADS), lds, s, a, f->ctx->tw);
  err = hipGetLastError();
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: launch: %s", who, hipGetErrorString(err));
  if (!ent.empty()) {
    const uint32_t bx = (uint32_t)((slot_floats + 255) / 256);
    hipLaunchKernelGGL(k_plfb_combine, dim3(bx, (uint32_t)(ent.size() / 3)), dim3(256), 0, s, f->prof.dev, (const float*)f->slots,
                       (const uint32_t*)(f->dev + ent_off), nchan_out, f->npol_out, f->nbin);
    err = hipGetLastError();
    if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: combine launch: %s", who, hipGetErrorString(err));
  }
  return DSPSR_AMD_OK;
}

extern "C" float* dspsr_amd_plfb_profile_dev(dspsr_amd_plfb* f) { return f ? f->prof.dev : nullptr; }

extern "C" int dspsr_amd_plfb_synch(dspsr_amd_plfb* f, float* profile_host)
{
  if (!f || !profile_host) return DSPSR_AMD_EINVAL;
  return sums_synch(f->ctx, f->prof, profile_host, "dspsr_amd_plfb_synch");
}
