// Cyclic-spectrum folding (dspsr -cyclic): dsp::CyclicFold / dsp::CyclicFoldEngine on the device.
//
// Semantics: the reference's CPU engine (Signal/Pulsar/CyclicFold.C:293-301 plan, :339-448 fold).  For idat < ndat_fold - nlag
// and ilag < nlag:   lag[bin][pol][chan][ilag] += x[idat] * conj(y[idat + ilag]),   bin = plan[ilag % 2][idat + ilag / 2].
//
// The kernel walks SKEWED time u = idat + ilag / 2.  In u the bin of a product depends on the parity of the lag alone, so all
// lags of one parity change bin at the same step: a wave holds 64 lags of ONE parity, its bin changes are wave-uniform, and
// the two run lists (one per parity, built on the host from the per-sample plans) drive the loop -- no plan lookup and no
// compare per sample.  A lane owns one lag and all products of it; with h = ilag / 2, par = ilag % 2 it needs
// x[u - h] and y[u + h + par], consecutive across the lanes of a wave in opposite directions: conflict-free 8-byte LDS reads
// from a window of T + 64 samples of every polarisation that the workgroup stages once per tile of T steps.  Samples
// outside the reference's ranges (idat outside [0, ndat_fold - nlag), idat + ilag outside the block) are staged as zeros,
// so they add +0 and the loop needs no edge cases.
//
// A workgroup is (128 lags, one channel, one time SEGMENT).  Accumulators live in registers for the length of a run and are
// added to memory when the run ends: (chan, lag, segment) has exactly one owner lane, and every segment adds into a partial
// lag array of its own, so there is no atomic and no race.  dspsr_amd_cyclic_fold_lagdata_dev adds the partial arrays in
// segment order (k_cyclic_combine).  The number of partial arrays is a function of the shape alone (never of the device or
// of timing): results are the same bits run to run, and the same for the same sequence of fold calls.
#include <math.h>
#include <string.h>

#include <vector>

#include "engine_internal.h"

namespace dspsr_amd {

constexpr int CY_T = 512;        // steps of u per tile
constexpr int CY_HL = 64;        // half-lags per workgroup: 128 lags = one wave of even lags and one wave of odd ones
constexpr int CY_THREADS = 128;
constexpr uint32_t CY_TARGET_WG = 1024;                   // workgroups wanted per launch when time has to be cut
constexpr uint32_t CY_MAX_PARTS = 64;
constexpr uint64_t CY_PART_BYTES = 2ull << 30;            // the partial lag arrays together take at most this
constexpr uint32_t CY_MAX_NLAG = 1u << 16;

struct CyclicArgs {
  const float* in;                // row (chan, pol) = in + chan * cs + pol * ps, first sample of the fold (idat_start applied)
  uint64_t cs, ps;
  float* parts;                   // partial lag arrays, part_floats apart
  uint64_t part_floats;
  const uint32_t* run_end[2];     // per parity: exclusive end (in u) of every run
  const uint32_t* run_bin[2];     //             its bin
  const uint32_t* tile_first[2];  //             the run that holds the first step of every tile
  uint32_t nvalid;                // ndat_fold - nlag: x samples that take part
  uint32_t ndat;                  // ndat_fold: y samples of the block
  uint32_t nu;                    // steps of u: nvalid + (nlag - 1) / 2
  uint32_t nlag, nchan;
  uint32_t ntile, tiles_per_seg;
};

__device__ __forceinline__ void cmac(float2& acc, const float2 a, const float2 b)   // acc += a * conj(b)
{
  acc.x = fmaf(a.x, b.x, fmaf(a.y, b.y, acc.x));
  acc.y = fmaf(a.y, b.x, fmaf(-a.x, b.y, acc.y));
}

template <int NPI, int NPO>
__global__ __launch_bounds__(CY_THREADS) void k_cyclic_fold(const CyclicArgs a)
{
  __shared__ float2 X[NPI][CY_T + CY_HL];
  __shared__ float2 Y[NPI][CY_T + CY_HL + 1];
  const uint32_t tid = threadIdx.x;
  const uint32_t par = __builtin_amdgcn_readfirstlane(tid >> 6), hl = tid & 63;
  const uint32_t h0 = blockIdx.x * CY_HL;                 // first half-lag of the workgroup
  const uint32_t ilag = 2 * (h0 + hl) + par;
  const uint32_t chan = blockIdx.y, seg = blockIdx.z;
  const bool wave_active = 2 * h0 + par < a.nlag;         // wave-uniform
  const bool lane_active = ilag < a.nlag;
  const uint32_t tile_begin = seg * a.tiles_per_seg;
  const uint32_t tile_end = min(tile_begin + a.tiles_per_seg, a.ntile);
  if (tile_begin >= tile_end) return;

  const float* row[NPI];
#pragma unroll
  for (int p = 0; p < NPI; p++) row[p] = a.in + chan * a.cs + p * a.ps;
  const uint32_t* __restrict__ rend = a.run_end[par];
  const uint32_t* __restrict__ rbin = a.run_bin[par];
  uint32_t r = __builtin_amdgcn_readfirstlane(a.tile_first[par][tile_begin]);

  float2 acc[NPO];
#pragma unroll
  for (int q = 0; q < NPO; q++) acc[q] = make_float2(0.f, 0.f);
  bool open = false;                                       // acc holds products of run r (wave-uniform)
  float* const part = a.parts + (size_t)seg * a.part_floats;
  const size_t pol_floats = (size_t)a.nchan * a.nlag * 2;
  const size_t own = ((size_t)chan * a.nlag + ilag) * 2;

  auto flush = [&](const uint32_t bin) {
    if (lane_active) {
#pragma unroll
      for (int q = 0; q < NPO; q++) {
        float2* dst = reinterpret_cast<float2*>(part + ((size_t)bin * NPO + q) * pol_floats + own);
        float2 v = *dst;
        v.x += acc[q].x;
        v.y += acc[q].y;
        *dst = v;
      }
    }
#pragma unroll
    for (int q = 0; q < NPO; q++) acc[q] = make_float2(0.f, 0.f);
  };

  for (uint32_t tile = tile_begin; tile < tile_end; tile++) {
    const uint32_t u0 = tile * CY_T;
    __syncthreads();
    // X[p][i] = x[u0 - (h0 + 63) + i], Y[p][i] = y[u0 + h0 + i]; zeros outside the ranges the reference multiplies
    const int64_t xbase = (int64_t)u0 - (int64_t)(h0 + CY_HL - 1);
    const uint64_t ybase = (uint64_t)u0 + h0;
    for (uint32_t i = tid; i < CY_T + CY_HL + 1; i += CY_THREADS) {
      const int64_t ix = xbase + i;
      const uint64_t iy = ybase + i;
      const bool okx = i < CY_T + CY_HL && ix >= 0 && ix < (int64_t)a.nvalid;
      const bool oky = iy < a.ndat;
#pragma unroll
      for (int p = 0; p < NPI; p++) {
        if (i < CY_T + CY_HL) X[p][i] = okx ? reinterpret_cast<const float2*>(row[p])[ix] : make_float2(0.f, 0.f);
        Y[p][i] = oky ? reinterpret_cast<const float2*>(row[p])[iy] : make_float2(0.f, 0.f);
      }
    }
    __syncthreads();
    if (!wave_active) continue;
    const uint32_t uend = min(u0 + CY_T, a.nu);
    const float2* x0 = &X[0][CY_HL - 1 - hl];
    const float2* y0 = &Y[0][hl + par];
    const float2* x1 = &X[NPI - 1][CY_HL - 1 - hl];
    const float2* y1 = &Y[NPI - 1][hl + par];
    uint32_t u = u0;
    while (u < uend) {
      const uint32_t re = __builtin_amdgcn_readfirstlane(rend[r]);
      const uint32_t e = min(re, uend);
      for (uint32_t j = u - u0; j < e - u0; j++) {
        const float2 xa = x0[j], ya = y0[j];
        if (NPI == 1) {
          cmac(acc[0], xa, ya);
        } else {
          const float2 xb = x1[j], yb = y1[j];
          cmac(acc[0], xa, ya);
          cmac(acc[NPO == 1 ? 0 : 1], xb, yb);
          if (NPO == 4) {
            cmac(acc[NPO == 4 ? 2 : 0], xa, yb);
            cmac(acc[NPO == 4 ? 3 : 0], xb, ya);
          }
        }
      }
      open = true;
      u = e;
      if (re <= uend) {                                    // the run ends inside this tile
        flush(__builtin_amdgcn_readfirstlane(rbin[r]));
        open = false;
        r++;
      }
    }
  }
  if (wave_active && open) flush(__builtin_amdgcn_readfirstlane(rbin[r]));
}

// lag[i] = part 0 + part 1 + ... in segment order
__global__ __launch_bounds__(256) void k_cyclic_combine(float* __restrict__ out, const float* __restrict__ parts,
                                                        const uint64_t part_floats, const uint32_t nparts)
{
  const uint64_t n2 = part_floats / 2;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * blockDim.x) {
    float2 s = reinterpret_cast<const float2*>(parts)[i];
    for (uint32_t p = 1; p < nparts; p++) {
      const float2 v = reinterpret_cast<const float2*>(parts + p * part_floats)[i];
      s.x += v.x;
      s.y += v.y;
    }
    reinterpret_cast<float2*>(out)[i] = s;
  }
}

}  // namespace dspsr_amd
using namespace dspsr_amd;

struct dspsr_amd_cyclic_fold {
  dspsr_amd_ctx* ctx = nullptr;
  uint32_t nchan = 0, npol_in = 0, npol_out = 0, nlag = 0, mover = 1, nbin = 0;
  uint32_t nparts = 0;
  uint64_t lag_floats = 0;
  float* parts = nullptr;         // nparts partial lag arrays
  float* lagdata = nullptr;       // their sum (== parts when nparts == 1)
  bool dirty = false;             // parts changed since the last combine
  uint64_t ndat_fold = 0, idat_start = 0;
  bool block_set = false;         // set_ndat came after the last change of shape: plan[] and ndat_fold belong to this shape
  std::vector<uint32_t> plan[2];  // per-sample plans of the current call (CyclicFold.C:293-301)
  std::vector<uint32_t> host;     // run lists as uploaded
  uint32_t* dev = nullptr;
  size_t dev_count = 0;
};

static void cyclic_release(dspsr_amd_cyclic_fold* f)
{
  (void)hipStreamSynchronize(f->ctx->stream);
  if (f->lagdata && f->lagdata != f->parts) (void)hipFree(f->lagdata);
  if (f->parts) (void)hipFree(f->parts);
  f->parts = f->lagdata = nullptr;
  f->lag_floats = 0;
  f->nparts = 0;
}

extern "C" int dspsr_amd_cyclic_fold_create(dspsr_amd_ctx* ctx, dspsr_amd_cyclic_fold** out)
{
  if (!ctx || !out) return DSPSR_AMD_EINVAL;
  dspsr_amd_cyclic_fold* f = new dspsr_amd_cyclic_fold;
  f->ctx = ctx;
  *out = f;
  return DSPSR_AMD_OK;
}

extern "C" void dspsr_amd_cyclic_fold_destroy(dspsr_amd_cyclic_fold* f)
{
  if (!f) return;
  cyclic_release(f);
  if (f->dev) (void)hipFree(f->dev);
  delete f;
}

extern "C" int dspsr_amd_cyclic_fold_set_shape(dspsr_amd_cyclic_fold* f, uint32_t nchan, uint32_t npol_in, uint32_t npol_out,
                                               uint32_t nlag, uint32_t mover, uint32_t nbin)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_cyclic_fold_set_shape";
  if (!nchan || !nbin || nlag < 2 || !mover) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: zero dimension or nlag < 2", who);
  if (npol_in != 1 && npol_in != 2) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: npol_in=%u not 1 or 2", who, npol_in);
  if (npol_out != 1 && npol_out != 2 && npol_out != 4)      // CyclicFold.C:106-119
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: invalid npol=%u", who, npol_out);
  if (npol_in == 1 && npol_out != 1)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: one input polarisation gives npol_out = 1 only (got %u)", who, npol_out);
  if (nlag > CY_MAX_NLAG || nchan > 65535)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: nlag=%u > %u or nchan=%u > 65535", who, nlag, CY_MAX_NLAG, nchan);
  if ((2 * nlag - 2) % mover) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: 2*nlag-2 is no multiple of mover=%u", who, mover);
  const uint64_t need = (uint64_t)nbin * npol_out * nchan * nlag * 2;
  // how many time segments (partial arrays): enough workgroups to fill the chip, within the memory set aside for them
  const uint32_t owners = nchan * ((nlag + 2 * CY_HL - 1) / (2 * CY_HL));
  uint32_t nparts = (CY_TARGET_WG + owners - 1) / owners;
  if (nparts > CY_MAX_PARTS) nparts = CY_MAX_PARTS;
  const uint64_t cap = CY_PART_BYTES / (need * sizeof(float));
  if (nparts > cap) nparts = (uint32_t)cap;
  if (nparts < 1) nparts = 1;
  const bool changed = nchan != f->nchan || npol_in != f->npol_in || npol_out != f->npol_out || nlag != f->nlag ||
                       mover != f->mover || nbin != f->nbin;
  if (changed) {
    // the plan of the previous shape holds bins of ITS nbin over ITS block: a fold must not launch with it
    f->plan[0].clear();
    f->plan[1].clear();
    f->ndat_fold = 0;
    f->block_set = false;
  }
  if (need != f->lag_floats || nparts != f->nparts) {
    cyclic_release(f);
    if (hipMalloc((void**)&f->parts, need * nparts * sizeof(float)) != hipSuccess) {
      f->parts = nullptr;
      return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc(%llu floats x %u) failed", who, (unsigned long long)need, nparts);
    }
    f->lagdata = f->parts;
    if (nparts > 1 && hipMalloc((void**)&f->lagdata, need * sizeof(float)) != hipSuccess) {
      (void)hipFree(f->parts);
      f->parts = f->lagdata = nullptr;
      return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc(%llu floats) failed", who, (unsigned long long)need);
    }
    f->lag_floats = need;
    f->nparts = nparts;
    (void)hipMemsetAsync(f->parts, 0, need * nparts * sizeof(float), f->ctx->stream);
    if (f->lagdata != f->parts) (void)hipMemsetAsync(f->lagdata, 0, need * sizeof(float), f->ctx->stream);
    f->dirty = false;
  } else if (changed) {
    // same size, another meaning (nbin and nchan exchanged, say): a new shape starts from zero like a new allocation
    const int rc = dspsr_amd_cyclic_fold_zero(f);
    if (rc != DSPSR_AMD_OK) return rc;
  }
  f->nchan = nchan; f->npol_in = npol_in; f->npol_out = npol_out; f->nlag = nlag; f->mover = mover; f->nbin = nbin;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_cyclic_fold_set_ndat(dspsr_amd_cyclic_fold* f, uint64_t ndat, uint64_t idat_start)   // CyclicFold.C:234-256
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (ndat >= (1ull << 31)) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_cyclic_fold_set_ndat: ndat=%llu >= 2^31",
                                            (unsigned long long)ndat);
  f->plan[0].assign(ndat, 0);
  f->plan[1].assign(ndat, 0);
  f->ndat_fold = ndat;
  f->idat_start = idat_start;
  f->block_set = true;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_cyclic_fold_set_bin(dspsr_amd_cyclic_fold* f, uint64_t idat, double ibin, double bins_per_sample)
{
  if (!f) return DSPSR_AMD_EINVAL;                          // CyclicFold.C:293-301
  if (!f->nbin) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_cyclic_fold_set_bin: no shape");
  if (idat < f->idat_start || idat - f->idat_start >= f->ndat_fold)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_cyclic_fold_set_bin: idat=%llu outside the block", (unsigned long long)idat);
  const uint32_t b0 = (uint32_t)ibin, b1 = (uint32_t)(ibin + 0.5 * bins_per_sample) % f->nbin;
  if (b0 >= f->nbin) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_cyclic_fold_set_bin: ibin=%u >= nbin", b0);
  f->plan[0][idat - f->idat_start] = b0;
  f->plan[1][idat - f->idat_start] = b1;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_cyclic_fold_set_bins(dspsr_amd_cyclic_fold* f, double phi, double phase_per_sample, uint64_t ndat,
                                              uint64_t idat_start, uint32_t* hits_host, uint64_t* ndat_folded)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->nbin) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_cyclic_fold_set_bins: no shape");
  if (idat_start < f->idat_start || idat_start - f->idat_start + ndat > f->ndat_fold)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_cyclic_fold_set_bins: samples outside the block of set_ndat");
  const uint64_t o = idat_start - f->idat_start;
  const int rc = dspsr_amd_cyclic_binplan(phi, phase_per_sample, f->nbin, ndat, f->plan[0].data() + o, f->plan[1].data() + o,
                                          hits_host);
  if (rc != DSPSR_AMD_OK) return ctx_fail(f->ctx, rc, "dspsr_amd_cyclic_fold_set_bins: the plan left [0, nbin)");
  if (ndat_folded) *ndat_folded = ndat;                     // Fold.C:783-784: every sample counts
  return DSPSR_AMD_OK;
}

template <int NPI, int NPO>
static void cyclic_launch(const dim3 grid, hipStream_t s, const CyclicArgs& a)
{
  hipLaunchKernelGGL((k_cyclic_fold<NPI, NPO>), grid, dim3(CY_THREADS), 0, s, a);
}

extern "C" int dspsr_amd_cyclic_fold_fold(dspsr_amd_cyclic_fold* f, const float* in_dev, uint64_t in_chan_stride,
                                          uint64_t in_pol_stride)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_cyclic_fold_fold";
  if (!f->parts) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
  if (!f->block_set)
    return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no block: dspsr_amd_cyclic_fold_set_ndat must follow a set_shape that changes the shape",
                    who);
  if (f->ndat_fold <= f->nlag) return DSPSR_AMD_OK;        // CyclicFold.C:358-367: a short block is ignored
  if (!in_dev) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: null input", who);
  const uint64_t row = 2 * (f->idat_start + f->ndat_fold);
  if (((uintptr_t)in_dev & 7) || (in_chan_stride & 1) || (in_pol_stride & 1))
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: rows must be 8-byte aligned (pointer %p, strides %llu, %llu floats)", who,
                    (const void*)in_dev, (unsigned long long)in_chan_stride, (unsigned long long)in_pol_stride);
  if ((f->npol_in > 1 && in_pol_stride < row) || (f->nchan > 1 && in_chan_stride < row))
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: stride shorter than the row of %llu floats", who, (unsigned long long)row);

  const uint32_t ndat = (uint32_t)f->ndat_fold, nlag = f->nlag;
  const uint32_t nvalid = ndat - nlag, nu = nvalid + (nlag - 1) / 2;
  const uint32_t ntile = (nu + CY_T - 1) / CY_T;
  const uint32_t nseg = f->nparts < ntile ? f->nparts : ntile;
  const uint32_t tps = (ntile + nseg - 1) / nseg;
  // run lists of the two plans over u in [0, ndat): ends, bins, first run of every tile
  size_t nrun[2];
  for (int p = 0; p < 2; p++) {
    nrun[p] = 1;
    const uint32_t* pl = f->plan[p].data();
    for (uint32_t i = 1; i < ndat; i++) nrun[p] += pl[i] != pl[i - 1];
  }
  f->host.resize(2 * (nrun[0] + nrun[1]) + 2 * (size_t)ntile);
  size_t off_end[2], off_bin[2], off_tile[2], o = 0;
  for (int p = 0; p < 2; p++) {
    off_end[p] = o; o += nrun[p];
    off_bin[p] = o; o += nrun[p];
    off_tile[p] = o; o += ntile;
    const uint32_t* pl = f->plan[p].data();
    uint32_t* e = f->host.data() + off_end[p];
    uint32_t* b = f->host.data() + off_bin[p];
    uint32_t* t = f->host.data() + off_tile[p];
    size_t r = 0;
    for (uint32_t i = 0; i < ndat; i++) {
      if (i && pl[i] != pl[i - 1]) e[r++] = i;
      if (i % CY_T == 0 && i / CY_T < ntile) t[i / CY_T] = (uint32_t)r;
      b[r] = pl[i];
    }
    e[r] = ndat;
  }
  hipStream_t s = f->ctx->stream;
  // the copy below reads f->host when it is issued (pageable memory: staged before the call returns), and launches in flight
  // may still read the lists of the previous call: the stream orders both
  if (!grow_device_buffer(s, f->dev, f->dev_count, f->host.size()))
    return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc(%zu run entries) failed", who, f->host.size());
  hipError_t err = hipMemcpyAsync(f->dev, f->host.data(), f->host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: plan upload: %s", who, hipGetErrorString(err));

  CyclicArgs a;
  a.in = in_dev + 2 * f->idat_start;
  a.cs = in_chan_stride; a.ps = in_pol_stride;
  a.parts = f->parts; a.part_floats = f->lag_floats;
  for (int p = 0; p < 2; p++) {
    a.run_end[p] = f->dev + off_end[p];
    a.run_bin[p] = f->dev + off_bin[p];
    a.tile_first[p] = f->dev + off_tile[p];
  }
  a.nvalid = nvalid; a.ndat = ndat; a.nu = nu; a.nlag = nlag; a.nchan = f->nchan;
  a.ntile = ntile; a.tiles_per_seg = tps;
  const dim3 grid((nlag + 2 * CY_HL - 1) / (2 * CY_HL), f->nchan, nseg);
  if (f->npol_in == 1) cyclic_launch<1, 1>(grid, s, a);
  else if (f->npol_out == 1) cyclic_launch<2, 1>(grid, s, a);
  else if (f->npol_out == 2) cyclic_launch<2, 2>(grid, s, a);
  else cyclic_launch<2, 4>(grid, s, a);
  err = hipGetLastError();
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: launch: %s", who, hipGetErrorString(err));
  f->dirty = true;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_cyclic_fold_zero(dspsr_amd_cyclic_fold* f)   // CyclicFold.C:283-291
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->parts) return DSPSR_AMD_OK;
  hipError_t e = hipMemsetAsync(f->parts, 0, f->lag_floats * f->nparts * sizeof(float), f->ctx->stream);
  if (e == hipSuccess && f->lagdata != f->parts) e = hipMemsetAsync(f->lagdata, 0, f->lag_floats * sizeof(float), f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_cyclic_fold_zero: %s", hipGetErrorString(e));
  f->dirty = false;
  return DSPSR_AMD_OK;
}

extern "C" float* dspsr_amd_cyclic_fold_lagdata_dev(dspsr_amd_cyclic_fold* f)
{
  if (!f || !f->parts) return nullptr;
  if (f->dirty && f->lagdata != f->parts) {
    const uint64_t n2 = f->lag_floats / 2;
    const uint32_t blocks = (uint32_t)((n2 + 255) / 256 < 4096 ? (n2 + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_cyclic_combine, dim3(blocks), dim3(256), 0, f->ctx->stream, f->lagdata, (const float*)f->parts,
                       f->lag_floats, f->nparts);
    if (hipGetLastError() != hipSuccess) return nullptr;
  }
  f->dirty = false;
  return f->lagdata;
}

extern "C" int dspsr_amd_cyclic_fold_synch_lags(dspsr_amd_cyclic_fold* f, float* lagdata_host)
{
  if (!f || !lagdata_host) return DSPSR_AMD_EINVAL;
  const float* src = dspsr_amd_cyclic_fold_lagdata_dev(f);
  if (!src) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_cyclic_fold_synch_lags: no lag data");
  hipError_t e = hipMemcpyAsync(lagdata_host, src, f->lag_floats * sizeof(float), hipMemcpyDeviceToHost, f->ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_cyclic_fold_synch_lags: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}
