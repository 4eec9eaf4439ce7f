// dsp::SpectralKurtosis on the device: estimate, detect, mask (Signal/General/SpectralKurtosis.C, the CPU branch in FPT order is the
// definition; where the reference's CUDA engines differ -- SKDetectorCUDA.cu averages the fscr sum over zapped channels too and its
// tscr detection races -- the CPU branch wins).  Input: complex rows [nchan][npol][ndat], ndim 2, as the filterbank writes them.
//   compute (:302-371)  per (part, chan, pol): S1 = sum |x|^2, S2 = sum |x|^4 over the M samples of the part, the estimate
//                       M_fac * (M * (S2 / (S1*S1)) - 1) in TFP order, and the same from the sums over all parts of the call (tscr)
//   detect  (:413-741)  reset_mask, detect_tscr, detect_skfb, detect_fscr, count_zapped on the small estimate array
//   mask    (:747-797)  out = mask[part][chan] ? 0 : in
// Every float operation that decides a zap is the reference's, one rounding each (__fmul_rn / __fadd_rn / __fdiv_rn / __fsqrt_rn: the
// reference is x86 host code without fused multiply-add), in the reference's order; only the sums over the M samples of one part are
// re-associated (k_sk_compute).  No float atomics anywhere: the same calls give the same bits.
#include "engine_internal.h"

#include <vector>

namespace dspsr_amd {

// lanes that share one (part, row) item: the pairs of samples of a part are dealt round-robin to W lanes, four pairs per lane
// where the part is short (four independent loads in flight per lane, a butterfly of four levels instead of six)
__host__ __device__ static inline uint32_t sk_lanes(const uint32_t M)
{
  const uint32_t P = (M + 1) / 2;
  return P <= 64 ? 16u : P <= 128 ? 32u : 64u;
}

// S1, S2 and the estimate of every (part, row), row = chan * npol + pol.  One pass over the rows.
//
// The sums run in a fixed tree that depends on M alone -- not on npart, the grid, the alignment or how a stream is cut into calls:
//   * the M samples of a part form P = ceil(M / 2) pairs (2j, 2j+1); W = sk_lanes(M) lanes share the part, 64 / W parts per wave;
//   * lane s takes the pairs j = s, s + W, s + 2W, ...; its k-th pair goes to accumulator k mod 4, first sample 2j, then 2j+1;
//   * the lane's sum is (a0 + a1) + (a2 + a3); the lanes are added in an xor butterfly, offsets W/2, ..., 1 (a + b == b + a, so every
//     lane holds the same bits and lane 0 stores).
// The longest chain of additions a term passes through is therefore
//   L(M) = 2 * ceil(ceil(P / W) / 4) - 1  +  2  +  log2(W)       (in the accumulator, across the four, across the lanes)
// e.g. L(32) = 7, L(128) = 7, L(1024) = 11, L(65536) = 263.  (The first addition of an accumulator is 0 + x, exact.)
// VEC: part starts are 16-byte aligned (M even, rows and strides 16-byte aligned) and a lane loads its pair as one float4; otherwise
// as two float2.  Both forms add the same terms in the same order: the same bits.  A missing last sample (M odd) adds +0.
// Items run row-major (consecutive waves read consecutive parts of one row); 64-bit item arithmetic (npart * rows may pass 2^32).
template <bool VEC>
__global__ __launch_bounds__(256) void k_sk_compute(const float* __restrict__ in, const uint64_t chan_stride, const uint64_t pol_stride,
                                                    const uint32_t nchan, const uint32_t npol, const uint32_t M, const uint64_t npart,
                                                    float* __restrict__ est, float* __restrict__ s1, float* __restrict__ s2)
{
  const uint32_t W = sk_lanes(M), G = 64 / W, P = (M + 1) / 2;
  const uint32_t lane = threadIdx.x & 63, sub = lane & (W - 1), grp = lane / W;
  const uint64_t nrows = (uint64_t)nchan * npol, nitems = nrows * npart;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const float M_fac = (float)((M + 1) / (M - 1)), fM = (float)M;               // :253: an unsigned integer division, kept
  for (uint64_t base = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * G; base < nitems; base += nwaves * G) {
    const uint64_t item = base + grp;
    const bool valid = item < nitems;
    const uint64_t row = valid ? item / npart : 0, part = valid ? item % npart : 0;
    float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
      const float* p = in + (row / npol) * chan_stride + (row % npol) * pol_stride + part * 2ull * M;
      for (uint32_t j0 = sub; j0 < P; j0 += 4 * W) {
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
          const uint32_t j = j0 + u * W;
          if (j < P) {
            float4 v;
            if (VEC) {
              v = ((const float4*)p)[j];
            } else {
              const float2 x = ((const float2*)p)[2 * j];
              const float2 y = 2 * j + 1 < M ? ((const float2*)p)[2 * j + 1] : make_float2(0.f, 0.f);
              v = make_float4(x.x, x.y, y.x, y.y);
            }
            const float q0 = __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));      // :321-323, one rounding each
            const float q1 = __fadd_rn(__fmul_rn(v.z, v.z), __fmul_rn(v.w, v.w));
            a1[u] = __fadd_rn(__fadd_rn(a1[u], q0), q1);
            a2[u] = __fadd_rn(__fadd_rn(a2[u], __fmul_rn(q0, q0)), __fmul_rn(q1, q1));
          }
        }
      }
    }
    float t1 = __fadd_rn(__fadd_rn(a1[0], a1[1]), __fadd_rn(a1[2], a1[3]));
    float t2 = __fadd_rn(__fadd_rn(a2[0], a2[1]), __fadd_rn(a2[2], a2[3]));
    for (uint32_t o = W >> 1; o; o >>= 1) {                                             // (every lane of the wave takes part)
      t1 = __fadd_rn(t1, __shfl_xor(t1, (int)o));
      t2 = __fadd_rn(t2, __shfl_xor(t2, (int)o));
    }
    if (valid && sub == 0) {
      const uint64_t o = part * nrows + row;                                            // TFP
      s1[o] = t1;
      s2[o] = t2;
      est[o] = t1 == 0.f ? 0.f : __fmul_rn(M_fac, __fsub_rn(__fmul_rn(fM, __fdiv_rn(t2, __fmul_rn(t1, t1))), 1.f));   // :334-337
    }
  }
}

// The estimate of the whole call (:352-371): one thread per row adds the per-part S1 / S2 in part order, as the reference's
// S1_tscr += S1_sum does (zeroed at every call, :246-250), with M_t = float(M * npart) and the float factor (M_t+1)/(M_t-1).
__global__ void k_sk_tscr(const float* __restrict__ s1, const float* __restrict__ s2, const uint64_t nrows, const uint64_t npart,
                          const float M_t, float* __restrict__ est_tscr)
{
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nrows) return;
  float S1 = 0.f, S2 = 0.f;
  for (uint64_t part = 0; part < npart; part++) {
    S1 = __fadd_rn(S1, s1[part * nrows + row]);
    S2 = __fadd_rn(S2, s2[part * nrows + row]);
  }
  const float M_fac = __fdiv_rn(__fadd_rn(M_t, 1.f), __fsub_rn(M_t, 1.f));
  est_tscr[row] = S1 == 0.f ? 0.f : __fmul_rn(M_fac, __fsub_rn(__fmul_rn(M_t, __fdiv_rn(S2, __fmul_rn(S1, S1))), 1.f));
}

// counters on the device (vector integer atomics): zap_counts[ZAP_ALL, ZAP_SKFB, ZAP_FSCR, ZAP_TSCR] (SpectralKurtosis.h:17-20)
enum { SK_ZAP_ALL = 0, SK_ZAP_SKFB = 1, SK_ZAP_FSCR = 2, SK_ZAP_TSCR = 3 };

// detect_tscr (:514-537): a channel of [chan_start, chan_end) with any polarisation outside [lower, upper] is zapped in all parts
__global__ void k_sk_detect_tscr(const float* __restrict__ est_tscr, const uint32_t nchan, const uint32_t npol, const uint64_t npart,
                                 const uint32_t chan_start, const uint32_t chan_end, const float lower, const float upper,
                                 uint8_t* __restrict__ mask, unsigned long long* __restrict__ counts)
{
  const uint32_t chan = chan_start + blockIdx.y;
  if (chan >= chan_end) return;
  bool zap = false;
  for (uint32_t ipol = 0; ipol < npol; ipol++) {
    const float V = est_tscr[(uint64_t)chan * npol + ipol];
    if (V > upper || V < lower) zap = true;
  }
  if (!zap) return;
  for (uint64_t part = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; part < npart; part += (uint64_t)gridDim.x * blockDim.x)
    mask[part * nchan + chan] = 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counts[SK_ZAP_TSCR], (unsigned long long)npart);
}

// detect_skfb (:557-583): any polarisation of (part, chan) outside [lower, upper] zaps it, over all channels; the count takes
// only chan_start < chan < chan_end (strict, :576)
__global__ void k_sk_detect_skfb(const float* __restrict__ est, const uint32_t nchan, const uint32_t npol, const uint64_t npart,
                                 const uint32_t chan_start, const uint32_t chan_end, const float lower, const float upper,
                                 uint8_t* __restrict__ mask, unsigned long long* __restrict__ counts)
{
  const uint64_t n = npart * nchan;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    bool zap = false;
    for (uint32_t ipol = 0; ipol < npol; ipol++) {
      const float V = est[i * npol + ipol];
      if (V > upper || V < lower) zap = true;
    }
    if (zap) {
      mask[i] = 1;
      const uint32_t chan = (uint32_t)(i % nchan);
      if (chan > chan_start && chan < chan_end) atomicAdd(&counts[SK_ZAP_SKFB], 1ull);
    }
  }
}

// detect_fscr (:694-741): one thread per (part, pol) sums the estimates of the channels of the range that are not yet zapped,
// sequentially in channel order, in the reference's float operations; a part that fails in either polarisation is zapped in all
// channels.  The two polarisations of a part are neighbouring lanes: both read the mask before either writes it.
__global__ void k_sk_detect_fscr(const float* __restrict__ est, const uint32_t nchan, const uint32_t npol, const uint64_t npart,
                                 const uint32_t chan_start, const uint32_t chan_end, const float mu2, const float nsigma,
                                 uint8_t* mask, unsigned long long* __restrict__ counts)
{
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t part = t / npol;
  const uint32_t ipol = (uint32_t)(t % npol);
  int zap = 0;
  if (part < npart) {
    const float* e = est + part * nchan * npol;
    const uint8_t* m = mask + part * nchan;
    float sk_avg = 0.f;
    uint32_t cnt = 0;
    for (uint32_t chan = chan_start; chan < chan_end; chan++)
      if (m[chan] == 0) {
        sk_avg = __fadd_rn(sk_avg, e[(uint64_t)chan * npol + ipol]);
        cnt++;
      }
    if (cnt > 0) {
      sk_avg = __fdiv_rn(sk_avg, (float)cnt);
      const float one_sigma = __fsqrt_rn(__fdiv_rn(mu2, (float)cnt));
      const float up = __fadd_rn(1.f, __fmul_rn(nsigma, one_sigma));
      const float lo = __fsub_rn(1.f, __fmul_rn(nsigma, one_sigma));
      if (sk_avg > up || sk_avg < lo) zap = 1;
    }
  }
  if (npol == 2) zap |= __shfl_xor(zap, 1);                 // (blockDim.x is even: the pair shares a wave; a wave-wide exchange also
                                                            //  orders the reads above before the writes below)
  if (part < npart && zap) {
    for (uint32_t chan = ipol; chan < nchan; chan += npol) mask[part * nchan + chan] = 1;
    if (ipol == 0) atomicAdd(&counts[SK_ZAP_FSCR], (unsigned long long)nchan);
  }
}

// count_zapped (:639-664): one thread per channel of the range walks the parts in order; the float sums continue those of the
// earlier calls
__global__ void k_sk_count(const float* __restrict__ est, const uint8_t* __restrict__ mask, const uint32_t nchan, const uint32_t npol,
                           const uint64_t npart, const uint32_t chan_start, const uint32_t chan_end, float* __restrict__ filtered_sum,
                           float* __restrict__ unfiltered_sum, unsigned long long* __restrict__ filtered_hits,
                           unsigned long long* __restrict__ counts)
{
  const uint32_t chan = chan_start + blockIdx.x * blockDim.x + threadIdx.x;
  if (chan >= chan_end) return;
  float fs[2], us[2];
  for (uint32_t ipol = 0; ipol < npol; ipol++) {
    fs[ipol] = filtered_sum[chan * npol + ipol];
    us[ipol] = unfiltered_sum[chan * npol + ipol];
  }
  unsigned long long hits = 0, zapped = 0;
  for (uint64_t part = 0; part < npart; part++) {
    const uint64_t index = (part * nchan + chan) * npol;
    for (uint32_t ipol = 0; ipol < npol; ipol++) us[ipol] = __fadd_rn(us[ipol], est[index + ipol]);
    if (mask[part * nchan + chan] == 1) {
      zapped++;
      continue;
    }
    for (uint32_t ipol = 0; ipol < npol; ipol++) fs[ipol] = __fadd_rn(fs[ipol], est[index + ipol]);
    hits++;
  }
  for (uint32_t ipol = 0; ipol < npol; ipol++) {
    filtered_sum[chan * npol + ipol] = fs[ipol];
    unfiltered_sum[chan * npol + ipol] = us[ipol];
  }
  filtered_hits[chan] += hits;
  if (zapped) atomicAdd(&counts[SK_ZAP_ALL], zapped);
}

// mask, out of place (:773-796): copies or zeroes every sample of the npart * M that the estimates cover
__global__ void k_sk_mask(const uint8_t* __restrict__ mask, const float* __restrict__ in, const uint64_t in_chan_stride,
                          const uint64_t in_pol_stride, float* __restrict__ out, const uint64_t out_chan_stride,
                          const uint64_t out_pol_stride, const uint32_t nchan, const uint32_t npol, const uint32_t M, const uint64_t npart)
{
  const uint64_t ndat = npart * M;
  for (uint32_t row = blockIdx.y; row < nchan * npol; row += gridDim.y) {
    const uint32_t chan = row / npol, ipol = row % npol;
    const float2* p = (const float2*)(in + chan * in_chan_stride + ipol * in_pol_stride);
    float2* q = (float2*)(out + chan * out_chan_stride + ipol * out_pol_stride);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ndat; i += (uint64_t)gridDim.x * blockDim.x)
      q[i] = mask[(i / M) * nchan + chan] ? make_float2(0.f, 0.f) : p[i];
  }
}

// mask, in place: writes zeros over the zapped parts only and reads nothing but the mask.  One workgroup per (part, chan) in turn.
__global__ void k_sk_mask_zero(const uint8_t* __restrict__ mask, float* __restrict__ out, const uint64_t chan_stride,
                               const uint64_t pol_stride, const uint32_t nchan, const uint32_t npol, const uint32_t M, const uint64_t npart)
{
  const uint64_t n = npart * nchan;
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    if (!mask[i]) continue;
    const uint64_t part = i / nchan, chan = i % nchan;
    for (uint32_t ipol = 0; ipol < npol; ipol++) {
      float2* q = (float2*)(out + chan * chan_stride + ipol * pol_stride) + part * M;
      for (uint32_t j = threadIdx.x; j < M; j += blockDim.x) q[j] = make_float2(0.f, 0.f);
    }
  }
}

}  // namespace dspsr_amd
using namespace dspsr_amd;

struct sk_limit_pair {
  uint64_t m;
  uint32_t std_devs;
  float lower, upper;
};

struct dspsr_amd_sk {
  dspsr_amd_ctx* ctx = nullptr;
  uint32_t nchan = 0, npol = 0, M = 0;
  uint32_t std_devs = 3, chan_start = 0, chan_end = 0;      // chan_end 0: nchan (SpectralKurtosis.C:419-420)
  bool no_fscr = false, no_tscr = false, no_ft = false;
  uint64_t npart = 0;                                       // of the last compute
  float *est = nullptr, *s1 = nullptr, *s2 = nullptr;       // [npart][nchan][npol]
  size_t est_count = 0, s1_count = 0, s2_count = 0;
  uint8_t* mask = nullptr;                                  // [npart][nchan]
  size_t mask_count = 0;
  float* est_tscr = nullptr;                                // [nchan][npol]
  float *filtered_sum = nullptr, *unfiltered_sum = nullptr; // [nchan][npol]
  unsigned long long* filtered_hits = nullptr;              // [nchan]
  unsigned long long* counts = nullptr;                     // zap_counts[4]
  uint64_t npart_total = 0, unfiltered_hits = 0;
  std::vector<sk_limit_pair> limits;                        // per distinct (M or M * npart, std_devs): :476-501
};

static void sk_release(dspsr_amd_sk* f)
{
  (void)hipStreamSynchronize(f->ctx->stream);
  void* all[] = {f->est, f->s1, f->s2, f->mask, f->est_tscr, f->filtered_sum, f->unfiltered_sum, f->filtered_hits, f->counts};
  for (void* p : all)
    if (p) (void)hipFree(p);
  f->est = f->s1 = f->s2 = f->est_tscr = f->filtered_sum = f->unfiltered_sum = nullptr;
  f->mask = nullptr;
  f->filtered_hits = f->counts = nullptr;
  f->est_count = f->s1_count = f->s2_count = f->mask_count = 0;
  f->nchan = f->npol = f->M = 0;
  f->npart = 0;
}

static int sk_launched(dspsr_amd_sk* f, const char* who)
{
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

static inline uint32_t sk_chan_end(const dspsr_amd_sk* f) { return f->chan_end ? f->chan_end : f->nchan; }

// the rows [nchan][npol] of `row` floats at the given strides: aligned, no shorter than the row, and none overlapping another
static int sk_check_rows(dspsr_amd_sk* f, const char* who, const char* what, const float* p, const uint64_t cs, const uint64_t ps,
                         const uint64_t row)
{
  if (((uintptr_t)p & 7) || (f->nchan > 1 && (cs & 1)) || (f->npol > 1 && (ps & 1)))
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: %s rows must be 8-byte aligned (address %p, strides %llu, %llu floats)", who, what,
                    (const void*)p, (unsigned long long)cs, (unsigned long long)ps);
  if ((f->nchan > 1 && cs < row) || (f->npol > 1 && ps < row))
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: %s stride shorter than the row of %llu floats", who, what, (unsigned long long)row);
  if (f->nchan > 1 && f->npol > 1 && cs < (f->npol - 1) * ps + row && ps < (f->nchan - 1) * cs + row)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: %s rows overlap (strides %llu, %llu floats, row %llu)", who, what, (unsigned long long)cs,
                    (unsigned long long)ps, (unsigned long long)row);
  return DSPSR_AMD_OK;
}

static uint64_t sk_extent(const dspsr_amd_sk* f, const uint64_t cs, const uint64_t ps, const uint64_t row)
{
  return (f->nchan - 1) * cs + (f->npol - 1) * ps + row;
}

// the pair of dspsr_amd_sk_limits for m samples, computed once per distinct (m, std_devs)
static int sk_cached_limits(dspsr_amd_sk* f, const uint64_t m, const uint32_t m_arg, float* lower, float* upper)
{
  for (const sk_limit_pair& l : f->limits)
    if (l.m == m && l.std_devs == f->std_devs) {
      *lower = l.lower;
      *upper = l.upper;
      return DSPSR_AMD_OK;
    }
  if (dspsr_amd_sk_limits(m_arg, f->std_devs, lower, upper) != DSPSR_AMD_OK)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_sk_transform: dspsr_amd_sk_limits(%u, %u) refused", m_arg, f->std_devs);
  f->limits.push_back({m, f->std_devs, *lower, *upper});
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_sk_create(dspsr_amd_ctx* ctx, dspsr_amd_sk** out)
{
  if (!ctx || !out) return DSPSR_AMD_EINVAL;
  dspsr_amd_sk* f = new dspsr_amd_sk;
  f->ctx = ctx;
  *out = f;
  return DSPSR_AMD_OK;
}

extern "C" void dspsr_amd_sk_destroy(dspsr_amd_sk* f)
{
  if (!f) return;
  sk_release(f);
  delete f;
}

extern "C" int dspsr_amd_sk_set_shape(dspsr_amd_sk* f, uint32_t nchan, uint32_t npol, uint32_t M)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_sk_set_shape";
  if (M < 32 || M > 65536)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: M=%u outside [32, 65536] (below 32 the Pearson IV limits do not exist)", who, M);
  if (npol != 1 && npol != 2) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: npol=%u not 1 or 2", who, npol);
  if (!nchan || nchan > 65535) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: nchan=%u outside [1, 65535]", who, nchan);
  if (f->chan_end > nchan)
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: chan_end=%u of the options > nchan=%u", who, f->chan_end, nchan);
  if (nchan == f->nchan && npol == f->npol && M == f->M) return DSPSR_AMD_OK;
  sk_release(f);
  const size_t nrows = (size_t)nchan * npol;
  if (hipMalloc((void**)&f->est_tscr, nrows * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&f->filtered_sum, nrows * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&f->unfiltered_sum, nrows * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&f->filtered_hits, nchan * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc((void**)&f->counts, 4 * sizeof(unsigned long long)) != hipSuccess) {
    sk_release(f);
    return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc failed", who);
  }
  f->nchan = nchan; f->npol = npol; f->M = M;
  return dspsr_amd_sk_reset_count(f);
}

extern "C" int dspsr_amd_sk_reset_count(dspsr_amd_sk* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_sk_reset_count: no shape");
  const size_t nrows = (size_t)f->nchan * f->npol;
  hipError_t e = hipMemsetAsync(f->filtered_sum, 0, nrows * sizeof(float), f->ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->unfiltered_sum, 0, nrows * sizeof(float), f->ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->est_tscr, 0, nrows * sizeof(float), f->ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->filtered_hits, 0, f->nchan * sizeof(unsigned long long), f->ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->counts, 0, 4 * sizeof(unsigned long long), f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_sk_reset_count: %s", hipGetErrorString(e));
  f->npart_total = f->unfiltered_hits = 0;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_sk_set_options(dspsr_amd_sk* f, uint32_t std_devs, uint32_t chan_start, uint32_t chan_end, int no_fscr,
                                        int no_tscr, int no_ft)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_sk_set_options";
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
  if (std_devs == 0) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: std_devs == 0 (SKLimits::calc_limits invalid inputs)", who);
  if (chan_end > f->nchan) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: chan_end=%u > nchan=%u", who, chan_end, f->nchan);
  if (chan_start >= (chan_end ? chan_end : f->nchan))
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: chan_start=%u >= chan_end=%u", who, chan_start, chan_end ? chan_end : f->nchan);
  f->std_devs = std_devs; f->chan_start = chan_start; f->chan_end = chan_end;
  f->no_fscr = no_fscr != 0; f->no_tscr = no_tscr != 0; f->no_ft = no_ft != 0;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_sk_compute(dspsr_amd_sk* f, const float* in_dev, uint64_t chan_stride, uint64_t pol_stride, uint64_t ndat)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_sk_compute";
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
  if (!in_dev) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: null input", who);
  if (ndat >= (1ull << 31)) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: ndat=%llu >= 2^31", who, (unsigned long long)ndat);
  const uint64_t npart = ndat / f->M;                       // :204-205: the ndat % M samples behind are not touched
  const int rc = sk_check_rows(f, who, "input", in_dev, chan_stride, pol_stride, 2 * npart * f->M);
  if (rc != DSPSR_AMD_OK) return rc;
  f->npart = npart;
  if (!npart) return DSPSR_AMD_OK;                          // :224-225
  const uint64_t nrows = (uint64_t)f->nchan * f->npol, nitems = nrows * npart;
  if (!grow_device_buffer(f->ctx->stream, f->est, f->est_count, nitems) || !grow_device_buffer(f->ctx->stream, f->s1, f->s1_count, nitems) ||
      !grow_device_buffer(f->ctx->stream, f->s2, f->s2_count, nitems) ||
      !grow_device_buffer(f->ctx->stream, f->mask, f->mask_count, npart * f->nchan)) {
    f->npart = 0;
    return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc of the estimates of %llu parts failed", who, (unsigned long long)npart);
  }
  const uint32_t per_wg = 4 * (64 / sk_lanes(f->M));        // items of one workgroup in one turn
  uint64_t blocks = (nitems + per_wg - 1) / per_wg;
  const uint64_t cap = (uint64_t)(f->ctx->ncu ? f->ctx->ncu : 256) * 8;
  if (blocks > cap) blocks = cap;
  const bool vec = (f->M % 2) == 0 && ((uintptr_t)in_dev % 16) == 0 && (f->nchan == 1 || chan_stride % 4 == 0) &&
                   (f->npol == 1 || pol_stride % 4 == 0);
  if (vec)
    hipLaunchKernelGGL(k_sk_compute<true>, dim3((uint32_t)blocks), dim3(256), 0, f->ctx->stream, in_dev, chan_stride, pol_stride, f->nchan,
                       f->npol, f->M, npart, f->est, f->s1, f->s2);
  else
    hipLaunchKernelGGL(k_sk_compute<false>, dim3((uint32_t)blocks), dim3(256), 0, f->ctx->stream, in_dev, chan_stride, pol_stride, f->nchan,
                       f->npol, f->M, npart, f->est, f->s1, f->s2);
  if (!f->no_tscr)
    hipLaunchKernelGGL(k_sk_tscr, dim3((uint32_t)((nrows + 63) / 64)), dim3(64), 0, f->ctx->stream, f->s1, f->s2, nrows, npart,
                       (float)(f->M * npart), f->est_tscr);
  return sk_launched(f, who);
}

extern "C" int dspsr_amd_sk_reset_mask(dspsr_amd_sk* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_sk_reset_mask: no shape");
  if (!f->npart) return DSPSR_AMD_OK;
  const hipError_t e = hipMemsetAsync(f->mask, 0, f->npart * f->nchan, f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_sk_reset_mask: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_sk_detect_tscr(dspsr_amd_sk* f, float lower, float upper)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_sk_detect_tscr: no shape");
  if (!f->npart) return DSPSR_AMD_OK;
  const uint32_t ce = sk_chan_end(f);
  uint64_t bx = (f->npart + 255) / 256;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(k_sk_detect_tscr, dim3((uint32_t)bx, ce - f->chan_start), dim3(256), 0, f->ctx->stream, f->est_tscr, f->nchan, f->npol,
                     f->npart, f->chan_start, ce, lower, upper, f->mask, f->counts);
  return sk_launched(f, "dspsr_amd_sk_detect_tscr");
}

extern "C" int dspsr_amd_sk_detect_skfb(dspsr_amd_sk* f, float lower, float upper)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_sk_detect_skfb: no shape");
  if (!f->npart) return DSPSR_AMD_OK;
  uint64_t bx = (f->npart * f->nchan + 255) / 256;
  if (bx > 4096) bx = 4096;
  hipLaunchKernelGGL(k_sk_detect_skfb, dim3((uint32_t)bx), dim3(256), 0, f->ctx->stream, f->est, f->nchan, f->npol, f->npart,
                     f->chan_start, sk_chan_end(f), lower, upper, f->mask, f->counts);
  return sk_launched(f, "dspsr_amd_sk_detect_skfb");
}

extern "C" int dspsr_amd_sk_detect_fscr(dspsr_amd_sk* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_sk_detect_fscr: no shape");
  if (!f->npart) return DSPSR_AMD_OK;
  const float _M = (float)f->M;
  const float mu2 = (4 * _M * _M) / ((_M - 1) * (_M + 2) * (_M + 3));        // :672-673, in float as written
  const float nsigma = (float)(1 + f->std_devs);                             // :716-717: (1+std_devs) is an unsigned
  const uint64_t n = f->npart * f->npol;
  hipLaunchKernelGGL(k_sk_detect_fscr, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, f->ctx->stream, f->est, f->nchan, f->npol, f->npart,
                     f->chan_start, sk_chan_end(f), mu2, nsigma, f->mask, f->counts);
  return sk_launched(f, "dspsr_amd_sk_detect_fscr");
}

extern "C" int dspsr_amd_sk_count_zapped(dspsr_amd_sk* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_sk_count_zapped: no shape");
  if (!f->npart) return DSPSR_AMD_OK;
  f->npart_total += f->npart * f->nchan;                    // :434
  f->unfiltered_hits += f->npart;                           // :641
  const uint32_t ce = sk_chan_end(f);
  hipLaunchKernelGGL(k_sk_count, dim3((ce - f->chan_start + 63) / 64), dim3(64), 0, f->ctx->stream, f->est, f->mask, f->nchan, f->npol,
                     f->npart, f->chan_start, ce, f->filtered_sum, f->unfiltered_sum, f->filtered_hits, f->counts);
  return sk_launched(f, "dspsr_amd_sk_count_zapped");
}

extern "C" int dspsr_amd_sk_mask(dspsr_amd_sk* f, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride, float* out_dev,
                                 uint64_t out_chan_stride, uint64_t out_pol_stride)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_sk_mask";
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
  if (!in_dev || !out_dev) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: null rows", who);
  const uint64_t row = 2 * f->npart * f->M;
  int rc = sk_check_rows(f, who, "input", in_dev, in_chan_stride, in_pol_stride, row);
  if (rc == DSPSR_AMD_OK) rc = sk_check_rows(f, who, "output", out_dev, out_chan_stride, out_pol_stride, row);
  if (rc != DSPSR_AMD_OK) return rc;
  const bool in_place = in_dev == out_dev;
  if (in_place && ((f->nchan > 1 && in_chan_stride != out_chan_stride) || (f->npol > 1 && in_pol_stride != out_pol_stride)))
    return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: in place with different strides: the rows partly overlap", who);
  if (!in_place && row) {
    const float *ie = in_dev + sk_extent(f, in_chan_stride, in_pol_stride, row), *oe = out_dev + sk_extent(f, out_chan_stride, out_pol_stride, row);
    if (in_dev < oe && out_dev < ie) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: input and output rows partly overlap", who);
  }
  if (!f->npart) return DSPSR_AMD_OK;
  if (in_place) {
    uint64_t bx = f->npart * f->nchan;
    if (bx > 65536) bx = 65536;
    hipLaunchKernelGGL(k_sk_mask_zero, dim3((uint32_t)bx), dim3(256), 0, f->ctx->stream, f->mask, out_dev, out_chan_stride, out_pol_stride,
                       f->nchan, f->npol, f->M, f->npart);
  } else {
    uint64_t bx = (f->npart * f->M + 255) / 256;
    if (bx > 4096) bx = 4096;
    const uint32_t rows = f->nchan * f->npol;
    hipLaunchKernelGGL(k_sk_mask, dim3((uint32_t)bx, rows > 65535 ? 65535 : rows), dim3(256), 0, f->ctx->stream, f->mask, in_dev,
                       in_chan_stride, in_pol_stride, out_dev, out_chan_stride, out_pol_stride, f->nchan, f->npol, f->M, f->npart);
  }
  return sk_launched(f, who);
}

// SpectralKurtosis::transformation (:194-232): compute, detect (:413-454), mask, with the limits of dspsr_amd_sk_limits
extern "C" int dspsr_amd_sk_transform(dspsr_amd_sk* f, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                                      float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride, uint64_t ndat)
{
  if (!f) return DSPSR_AMD_EINVAL;
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_sk_transform: no shape");
  if (!in_dev || !out_dev) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_sk_transform: null rows");
  int rc = dspsr_amd_sk_compute(f, in_dev, in_chan_stride, in_pol_stride, ndat);
  if (rc != DSPSR_AMD_OK || !f->npart) return rc;
  float lower = 0, upper = 0;
  rc = dspsr_amd_sk_reset_mask(f);
  if (rc == DSPSR_AMD_OK && !f->no_tscr) {
    const uint64_t m = f->M * f->npart;
    rc = sk_cached_limits(f, m, (uint32_t)(float)m, &lower, &upper);       // :472,493: SKLimits(M_tscr = float(m), std_devs)
    if (rc == DSPSR_AMD_OK) rc = dspsr_amd_sk_detect_tscr(f, lower, upper);
  }
  if (rc == DSPSR_AMD_OK && !f->no_ft) {
    rc = sk_cached_limits(f, f->M, f->M, &lower, &upper);
    if (rc == DSPSR_AMD_OK) rc = dspsr_amd_sk_detect_skfb(f, lower, upper);
  }
  if (rc == DSPSR_AMD_OK && !f->no_fscr) rc = dspsr_amd_sk_detect_fscr(f);
  if (rc == DSPSR_AMD_OK) rc = dspsr_amd_sk_count_zapped(f);
  if (rc == DSPSR_AMD_OK) rc = dspsr_amd_sk_mask(f, in_dev, in_chan_stride, in_pol_stride, out_dev, out_chan_stride, out_pol_stride);
  return rc;
}

extern "C" uint64_t dspsr_amd_sk_npart(dspsr_amd_sk* f) { return f ? f->npart : 0; }
extern "C" float* dspsr_amd_sk_estimates_dev(dspsr_amd_sk* f) { return f ? f->est : nullptr; }
extern "C" float* dspsr_amd_sk_estimates_tscr_dev(dspsr_amd_sk* f) { return f ? f->est_tscr : nullptr; }
extern "C" uint8_t* dspsr_amd_sk_zapmask_dev(dspsr_amd_sk* f) { return f ? f->mask : nullptr; }

extern "C" int dspsr_amd_sk_get_statistics(dspsr_amd_sk* f, uint64_t* counts, uint64_t* filtered_hits, float* filtered_sum,
                                           float* unfiltered_sum)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_sk_get_statistics";
  if (!f->M) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
  const size_t nrows = (size_t)f->nchan * f->npol;
  hipStream_t s = f->ctx->stream;
  hipError_t e = hipSuccess;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counters are 64-bit");
  if (counts) e = hipMemcpyAsync(counts, f->counts, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && filtered_hits) e = hipMemcpyAsync(filtered_hits, f->filtered_hits, f->nchan * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && filtered_sum) e = hipMemcpyAsync(filtered_sum, f->filtered_sum, nrows * sizeof(float), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && unfiltered_sum) e = hipMemcpyAsync(unfiltered_sum, f->unfiltered_sum, nrows * sizeof(float), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(e));
  if (counts) {
    counts[4] = f->npart_total;
    counts[5] = f->unfiltered_hits;
  }
  return DSPSR_AMD_OK;
}
