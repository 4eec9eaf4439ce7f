// Phase-locked filterbank (dspsr -G nbin): dsp::PhaseLockedFilterbank on the device.
//
// Semantics: the loop body of Signal/Pulsar/PhaseLockedFilterbank.C:254-297.  A WINDOW is (idat_start, bin): nchan complex
// samples (Analytic rows) or 2 nchan real samples (Nyquist rows) of every input channel and polarisation from idat_start on are
// transformed (forward, unnormalised), square-law detected and added into phase bin `bin` of output channel chan * nchan + k.
//
// A workgroup tile is wgfft's 16384 points: C = nchan complex points x T = 16384 / C columns, the columns being the (window,
// polarisation) pairs of T / 2 windows -- both polarisations of a window are the two halves of a thread's butterfly pair, as
// in k_tfp.  Nyquist rows are transformed as C complex points z[n] = x[2n] + i x[2n+1] followed by the Hermitian split (k_tfp's),
// never as a 2 C point transform.  The transform is staged in the exchange buffer; thread t then owns bins t, t + 512, ... (bin
// pairs (k, C - k) for Nyquist rows) of EVERY window of the tile and adds their detected products to register sums.
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

namespace dspsr_amd {

constexpr uint32_t PL_THREADS = 512;
constexpr uint32_t PL_TARGET_WG = 1024;                   // workgroups wanted per launch when the windows have to be cut
constexpr uint32_t PL_MAX_SEG = 256;
constexpr uint64_t PL_SLOT_BYTES = 256ull << 20;          // the slots of a launch together take at most this
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
__global__ __launch_bounds__(PL_THREADS) void k_plfb(const PlfbArgs a, const cf* __restrict__ tw)
{
  typedef FftPlan<LOGC> P;
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  uint32_t tid = threadIdx.x;
  constexpr uint32_t nt = PL_THREADS;
  constexpr int logT = 14 - LOGC, logTp = logT - 1;
  constexpr uint32_t Tp = 1u << logTp, C = 1u << LOGC;
  constexpr uint32_t NK = NDIM == 2 ? C : C / 2;            // bins (Analytic) or bin pairs (Nyquist) of a window
  constexpr int NB = NK > nt ? NK / nt : 1;                 //   ... of which a thread owns NB
  constexpr int NE = NDIM == 2 ? 1 : 2;
  const uint32_t ltw_off = lds_pad(PTS * nt) + 8;
  ltw_fill<LOGC>(lds, ltw_off, tw, tid, nt);
  const uint32_t chan = blockIdx.y, seg = blockIdx.x;
  const uint32_t w_begin = seg * a.wps, w_end = min(w_begin + a.wps, a.nwin);
  const float* const row0 = a.in + chan * a.cs;
  const float* const row1 = row0 + a.ps;
  const bool two = a.npol_in > 1;                           // one input polarisation: the second column of every pair is zero

  float wc[NB], ws[NB];                                     // Nyquist: w^k = exp(-i pi k / C) = (wc, -ws)
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const float x = (float)(threadIdx.x + j * nt) * __uint_as_float((uint32_t)(127 - (LOGC + 1)) << 23);   // k / 2C revolutions, exact
    wc[j] = __builtin_amdgcn_cosf(x);
    ws[j] = __builtin_amdgcn_sinf(x);
  }

  float acc[NB][NE][NPO];
#pragma unroll
  for (int j = 0; j < NB; j++)
#pragma unroll
    for (int e = 0; e < NE; e++)
#pragma unroll
      for (int q = 0; q < NPO; q++) acc[j][e][q] = 0.f;
  uint32_t cur = 0xffffffffu;                               // destination of the sums held (uniform); none yet

  // adds the sums to their destination -- this workgroup is its only owner in the launch -- and clears them
  auto flush = [&](const uint32_t d) {
    uint32_t t0 = threadIdx.x;
    asm volatile("" : "+v"(t0));                            // (loop-invariant addresses: keep them out of the tile loop's registers)
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const uint32_t k = t0 + j * nt;
      if (k < NK) {
#pragma unroll
        for (int e = 0; e < NE; e++) {
          const uint32_t bin = e == 0 ? k : (k ? C - k : C / 2);
          const size_t co = (size_t)chan * C + bin;
#pragma unroll
          for (int q = 0; q < NPO; q++) {
            if (d & PL_SLOT) {
              a.slots[((size_t)(d & ~PL_SLOT) * NPO + q) * a.nchan_out + co] = acc[j][e][q];
            } else {
              float* const dst = a.prof + (co * NPO + q) * a.nbin + d;
              *dst += acc[j][e][q];
            }
          }
        }
      }
#pragma unroll
      for (int e = 0; e < NE; e++)
#pragma unroll
        for (int q = 0; q < NPO; q++) acc[j][e][q] = 0.f;
    }
  };
  // the detected products of one bin: X0, X1 = (re, im) of the two polarisations
  auto detect = [&](float (&s)[NPO], const float r0, const float i0, const float r1, const float i1, const float sgn) {
    float p0 = r0 * r0; p0 += i0 * i0;                      // PhaseLockedFilterbank.C:275-276
    float p1 = r1 * r1; p1 += i1 * i1;
    if constexpr (NPO == 1) {
      s[0] += p0 + p1;
    } else {
      s[0] += p0;
      s[1] += p1;
      if constexpr (NPO == 4) {
        s[2] += r0 * r1 + i0 * i1;                          // :288-293
        s[NPO == 4 ? 3 : 0] += sgn * (r0 * i1 - i0 * r1);
      }
    }
  };

  for (uint32_t w0 = w_begin; w0 < w_end; w0 += Tp) {
    asm volatile("" : "+v"(tid));
    cx2 x[NPAIR];
#pragma unroll
    for (int g2 = 0; g2 < P::G1; g2 += 2)
#pragma unroll
      for (int i = 0; i < P::R1; i++) {
        const uint32_t el = first_stage_elem<LOGC>(tid, logT, g2, i);
        const uint32_t w = w0 + ((el & ((1u << logT) - 1)) >> 1), n = el >> logT;
        float2 v0 = make_float2(0.f, 0.f), v1 = make_float2(0.f, 0.f);
        if (w < w_end) {
          const uint32_t s = a.wstart[w];
          if constexpr (NDIM == 2) {
            v0 = reinterpret_cast<const float2*>(row0)[s + n];
            if (two) v1 = reinterpret_cast<const float2*>(row1)[s + n];
          } else {
            const size_t o = (size_t)s + 2 * n;             // any parity of s: two 4-byte loads
            v0 = make_float2(row0[o], row0[o + 1]);
            if (two) v1 = make_float2(row1[o], row1[o + 1]);
          }
        }
        cx2& d = x[(g2 / 2) * P::R1 + i];
        d.x = (v2f){v0.x, v1.x};
        d.y = (v2f){v0.y, v1.y};
      }
    // staged transform: one plane of C float4 per window, (Re p0, Re p1, Im p0, Im p1) (k_tfp's staging)
    float4* const stg = (float4*)lds;
    constexpr uint32_t plane = C + (Tp <= 64 ? 8u : 0u);
    auto store = [&](const uint32_t col, const uint32_t pp, const uint32_t pstride, auto& v) {
      constexpr int R = sizeof(v) / sizeof(v[0]);
      float4* const d = stg + (col >> 1) * plane + pp;
#pragma unroll
      for (int k = 0; k < R; k++) d[k * pstride] = make_float4(v[k].x[0], v[k].x[1], v[k].y[0], v[k].y[1]);
    };
    wgfft<LOGC, -1, true>(lds, ltw_off, tid, logT, x, store);
    __syncthreads();
    const uint32_t nw = min(Tp, w_end - w0);
    for (uint32_t c2 = 0; c2 < nw; c2++) {
      const uint32_t d = __builtin_amdgcn_readfirstlane(a.wdst[w0 + c2]);
      if (d != cur) {
        if (cur != 0xffffffffu) flush(cur);
        cur = d;
      }
      const float4* const pl = stg + c2 * plane;
      uint32_t t0 = threadIdx.x;
      asm volatile("" : "+v"(t0));
#pragma unroll
      for (int j = 0; j < NB; j++) {
        const uint32_t k = t0 + j * nt;
        if (k >= NK) continue;
        if constexpr (NDIM == 2) {
          const float4 z = pl[k];
          detect(acc[j][0], z.x, z.z, z.y, z.w, 1.f);
        } else {
          // X[k] = A + w^k B, X[C-k] = conj(A - w^k B); A = (Z[k] + conj Z[C-k]) / 2, B = (Z[k] - conj Z[C-k]) / 2i.  Bins 0 and
          // C/2 are their own mirrors: X[0] from Z[0] with w = 1, X[C/2] from Z[C/2] with w = -i
          const float4 zk = pl[k], zm = pl[k ? C - k : 0];
          const v2f zr = {zk.x, zk.y}, zi = {zk.z, zk.w}, mr = {zm.x, zm.y}, mi = {zm.z, zm.w};
          const v2f ar = 0.5f * (zr + mr), ai = 0.5f * (zi - mi);
          const v2f br = 0.5f * (zi + mi), bi = 0.5f * (mr - zr);
          const float c = wc[j], sn = ws[j];
          const v2f wr = c * br + sn * bi, wi = c * bi - sn * br;
          const v2f xr = ar + wr, xi = ai + wi;
          detect(acc[j][0], xr[0], xi[0], xr[1], xi[1], 1.f);
          if (k) {
            const v2f yr = ar - wr, yi = ai - wi;           // X[C-k] = (yr, -yi)
            detect(acc[j][NE - 1], yr[0], yi[0], yr[1], yi[1], -1.f);
          } else {
            const float4 zh = pl[C / 2];                    // X[C/2] = (Re Z, -Im Z)
            detect(acc[j][NE - 1], zh.x, zh.z, zh.y, zh.w, -1.f);
          }
        }
      }
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

static int msg_fail(char* msg, size_t len, const char* fmt, ...)
{
  if (msg && len) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, len, fmt, ap);
    va_end(ap);
  }
  return DSPSR_AMD_EINVAL;
}

}  // namespace dspsr_amd
using namespace dspsr_amd;

struct dspsr_amd_plfb {
  dspsr_amd_ctx* ctx = nullptr;
  uint32_t nchan_in = 0, npol_in = 0, ndim_in = 0, nchan = 0, npol_out = 0, nbin = 0;
  uint64_t prof_floats = 0;
  float* prof = nullptr;
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

static void plfb_release(dspsr_amd_plfb* f)
{
  (void)hipStreamSynchronize(f->ctx->stream);
  if (f->prof) (void)hipFree(f->prof);
  f->prof = nullptr;
  f->prof_floats = 0;
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
  plfb_release(f);
  if (f->slots) (void)hipFree(f->slots);
  if (f->dev) (void)hipFree(f->dev);
  delete f;
}

extern "C" int dspsr_amd_plfb_zero(dspsr_amd_plfb* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->prof) return DSPSR_AMD_OK;
  const hipError_t e = hipMemsetAsync(f->prof, 0, f->prof_floats * sizeof(float), f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_plfb_zero: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
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
  const uint64_t need = (uint64_t)nchan_in * nchan * npol_out * nbin;
  if (need != f->prof_floats) {
    plfb_release(f);
    if (hipMalloc((void**)&f->prof, need * sizeof(float)) != hipSuccess) {
      f->prof = nullptr;
      f->nbin = 0;
      return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_plfb_set_shape: hipMalloc(%llu floats) failed", (unsigned long long)need);
    }
    f->prof_floats = need;
  }
  f->nchan_in = nchan_in; f->npol_in = npol_in; f->ndim_in = ndim_in; f->nchan = nchan; f->npol_out = npol_out; f->nbin = nbin;
  return changed ? dspsr_amd_plfb_zero(f) : DSPSR_AMD_OK;   // a new shape starts from zero; the same shape keeps its sums
}

extern "C" int dspsr_amd_plfb_accumulate(dspsr_amd_plfb* f, const float* in_dev, uint64_t chan_stride, uint64_t pol_stride,
                                         uint64_t ndat, uint64_t nwin, const uint64_t* idat_start_host, const uint32_t* bin_host)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_plfb_accumulate";
  if (!f->prof) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
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
  // segments: whole tiles; enough workgroups to fill the chip, within the memory set aside for the slots (two per segment at most)
  const uint32_t ntile = (n + tp - 1) / tp;
  uint32_t nseg = PL_TARGET_WG / f->nchan_in;
  if (nseg > PL_MAX_SEG) nseg = PL_MAX_SEG;
  const uint64_t slot_floats = (uint64_t)f->npol_out * nchan_out;
  const uint64_t cap = PL_SLOT_BYTES / (2 * slot_floats * sizeof(float));
  if (nseg > cap) nseg = (uint32_t)cap;
  if (nseg > ntile) nseg = ntile;
  if (nseg < 1) nseg = 1;
  const uint32_t wps = ((ntile + nseg - 1) / nseg) * tp;
  nseg = (n + wps - 1) / wps;

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
  a.prof = f->prof; a.slots = f->slots;
  a.wstart = f->dev; a.wdst = f->dev + n;
  a.nwin = n; a.wps = wps; a.nbin = f->nbin; a.nchan_out = nchan_out; a.npol_in = f->npol_in;
  const kplfb_t k = pick_plfb(logc, f->ndim_in, f->npol_out);
  const size_t lds = lds_total_words_host(16384, logc) * sizeof(cf);
  err = dspsr_amd_allow_lds((const void*)k, lds);
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(err));
  hipLaunchKernelGGL(k, dim3(nseg, f->nchan_in), dim3(PL_THREADS), lds, s, a, f->ctx->tw);
  err = hipGetLastError();
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: launch: %s", who, hipGetErrorString(err));
  if (!ent.empty()) {
    const uint32_t bx = (uint32_t)((slot_floats + 255) / 256);
    hipLaunchKernelGGL(k_plfb_combine, dim3(bx, (uint32_t)(ent.size() / 3)), dim3(256), 0, s, f->prof, (const float*)f->slots,
                       (const uint32_t*)(f->dev + ent_off), nchan_out, f->npol_out, f->nbin);
    err = hipGetLastError();
    if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: combine launch: %s", who, hipGetErrorString(err));
  }
  return DSPSR_AMD_OK;
}

extern "C" float* dspsr_amd_plfb_profile_dev(dspsr_amd_plfb* f) { return f ? f->prof : nullptr; }

extern "C" int dspsr_amd_plfb_synch(dspsr_amd_plfb* f, float* profile_host)
{
  if (!f || !profile_host) return DSPSR_AMD_EINVAL;
  if (!f->prof) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_plfb_synch: no shape");
  hipError_t e = hipMemcpyAsync(profile_host, f->prof, f->prof_floats * sizeof(float), hipMemcpyDeviceToHost, f->ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_plfb_synch: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
