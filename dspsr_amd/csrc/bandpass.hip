// Passband integration: dsp::Bandpass on the device (the operator behind dspsr -R's RFIFilter and the reference's passband tool).
//
// Semantics: the loop of Signal/General/Bandpass.C:122-162 with Response::integrate (Response.C:456-492, :587-612).  The input of
// every channel is cut into npart = ndat / nsamp_fft whole transforms -- contiguous, not overlapping, part k starts at sample
// k * nsamp_fft; nsamp_fft = 2 * resolution real samples (Nyquist) or resolution complex samples (Analytic); trailing samples
// that do not fill a transform are not read.  Each part is transformed (forward, unnormalised; Nyquist: bins 0 .. resolution - 1
// of the real-to-complex transform, the Nyquist bin dropped), detected -- re * re + im * im per polarisation, or PP, QQ, Re P* Q,
// Im P* Q (cross_detect_int) -- and added to pass[npol_out][nchan_in][resolution].
//
// The transform half is k_plfb's: a workgroup tile is wgfft's 16384 points, C = resolution complex points x 16384 / C columns, the
// columns being the (part, polarisation) pairs of Tp = 8192 / C parts; Nyquist rows are transformed as C packed complex points
// z[n] = x[2n] + i x[2n+1] followed by the Hermitian split; thread t owns bins t, t + 512, ... (bin pairs (k, C - k) for Nyquist rows)
// of every part of its tile.  New here: no window list; three input forms (float rows, the 8-bit block in the generic order, the
// 8-bit block in the CASPSR order, decoded as k_tfp decodes them: value = (int8 + 0.5) * scale); and one destination only.
//
// Accumulation: the parts of a call are cut into SEGMENTS of whole tiles.  Workgroup (segment, input channel) keeps its sums in
// registers over all tiles of its segment, in time order, and stores them once to partial[segment][npol_out][chan][C];
// k_bandpass_combine -- one owner per element -- adds the partial arrays to the passband in segment order.  The cut depends on
// (npart, nchan_in, resolution) alone and there are no atomics: the same calls give the same bits.
#include "engine_internal.h"

namespace dspsr_amd {

constexpr uint32_t BP_THREADS = 512;
constexpr uint32_t BP_TARGET_WG = 1024;                   // workgroups wanted per launch
constexpr uint32_t BP_MAX_SEG = 256;
constexpr uint64_t BP_PARTIAL_BYTES = 256ull << 20;       // the partial arrays of a launch take at most this, counted for npol_out = 4
                                                          // (set_shape refuses a shape whose ONE partial array would exceed it)

enum { BP_FLOAT = 0, BP_GENERIC = 1, BP_CASPSR = 2 };

struct BpArgs {
  const void* in;                 // float rows: element (chan, pol, t) = in + chan * cs + pol * ps + t * ndim; or the 8-bit block
  uint64_t cs, ps;
  float* partial;                 // [segment][npol_out][nchan_in][C]
  uint32_t npart, pps;            // parts of the call; parts per segment (a multiple of the tile's)
  uint32_t nchan_in, npol_in;
  float scale;
};

// The launch arithmetic (pure; tests/test_bandpass_cases_host.py restates it): parts per tile, tiles per segment, segments.
static void bp_cut(const uint32_t npart, const uint32_t nchan_in, const uint32_t resolution, uint32_t& tp, uint32_t& tps,
                   uint32_t& nseg)
{
  tp = 8192u / resolution;
  const uint32_t ntile = (npart + tp - 1) / tp;
  nseg = BP_TARGET_WG / nchan_in;
  if (nseg > BP_MAX_SEG) nseg = BP_MAX_SEG;
  const uint64_t cap = BP_PARTIAL_BYTES / (4ull * nchan_in * resolution * sizeof(float));
  if (nseg > cap) nseg = (uint32_t)cap;
  if (nseg > ntile) nseg = ntile;
  if (nseg < 1) nseg = 1;
  tps = (ntile + nseg - 1) / nseg;
  if (tps < 1) tps = 1;
  nseg = (ntile + tps - 1) / tps;
}

template <int LOGC, int NDIM, int NPO, int FORM>
__global__ __launch_bounds__(BP_THREADS) void k_bandpass(const BpArgs a, const cf* __restrict__ tw)
{
  typedef FftPlan<LOGC> P;
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  uint32_t tid = threadIdx.x;
  constexpr uint32_t nt = BP_THREADS;
  constexpr int logT = 14 - LOGC, logTp = logT - 1;
  constexpr uint32_t Tp = 1u << logTp, C = 1u << LOGC;
  constexpr uint32_t NK = NDIM == 2 ? C : C / 2;            // bins (Analytic) or bin pairs (Nyquist) of a part
  constexpr int NB = NK > nt ? NK / nt : 1;                 //   ... of which a thread owns NB
  constexpr int NE = NDIM == 2 ? 1 : 2;
  constexpr uint32_t NSAMP = NDIM == 2 ? C : 2 * C;         // samples of a part
  const uint32_t ltw_off = lds_pad(PTS * nt) + 8;
  ltw_fill<LOGC>(lds, ltw_off, tw, tid, nt);
  const uint32_t chan = blockIdx.y, seg = blockIdx.x;
  const uint32_t w_begin = seg * a.pps, w_end = min(w_begin + a.pps, a.npart);
  const bool two = a.npol_in > 1;                           // one input polarisation: the second column of every pair is zero
  const float hs = 0.5f * a.scale;

  // Nyquist: w^k = exp(-i pi k / C) = (wc, -ws), argument k / 2C revolutions, exact in float.  Held in registers across the tiles
  // where a thread owns few bin pairs; with NB = 8 (C = 8192: one part per tile) the 16 registers go to the sums instead and the two
  // values are evaluated per use -- the same instructions on the same argument, the same bits.
  constexpr bool HOLD_W = NB <= 4;
  auto wcos = [&](const uint32_t k) { return __builtin_amdgcn_cosf((float)k * __uint_as_float((uint32_t)(127 - (LOGC + 1)) << 23)); };
  auto wsin = [&](const uint32_t k) { return __builtin_amdgcn_sinf((float)k * __uint_as_float((uint32_t)(127 - (LOGC + 1)) << 23)); };
  float wc[HOLD_W ? NB : 1], ws[HOLD_W ? NB : 1];
  if constexpr (HOLD_W) {
#pragma unroll
    for (int j = 0; j < NB; j++) {
      wc[j] = wcos(threadIdx.x + j * nt);
      ws[j] = wsin(threadIdx.x + j * nt);
    }
  }

  float acc[NB][NE][NPO];
#pragma unroll
  for (int j = 0; j < NB; j++)
#pragma unroll
    for (int e = 0; e < NE; e++)
#pragma unroll
      for (int q = 0; q < NPO; q++) acc[j][e][q] = 0.f;

  // the detected products of one bin: P, Q = (re, im) of the two polarisations
  auto detect = [&](float (&s)[NPO], const float r0, const float i0, const float r1, const float i1, const float sgn) {
    float p0 = r0 * r0; p0 += i0 * i0;                      // Response.C:484-489
    if constexpr (NPO == 1) {
      s[0] += p0;
    } else {
      float p1 = r1 * r1; p1 += i1 * i1;
      s[0] += p0;
      s[1] += p1;
      if constexpr (NPO == 4) {
        s[2] += r0 * r1 + i0 * i1;                          // cross_detect.ic:39-40
        s[NPO == 4 ? 3 : 0] += sgn * (r0 * i1 - i0 * r1);
      }
    }
  };
  auto dec = [&](const uint32_t b) { return __builtin_fmaf((float)(int8_t)(b & 0xff), a.scale, hs); };

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
          const uint64_t s = (uint64_t)w * NSAMP;           // part w starts here: no window list
          if constexpr (FORM == BP_FLOAT) {
            const float* const row0 = (const float*)a.in + chan * a.cs;
            const float* const row1 = row0 + a.ps;
            const uint64_t o = (s << (NDIM - 1)) + 2 * n;   // any float address: two 4-byte loads
            v0 = make_float2(row0[o], row0[o + 1]);
            if (two) v1 = make_float2(row1[o], row1[o + 1]);
          } else if constexpr (FORM == BP_GENERIC) {
            // byte ((t * nchan + c) * npol + p) * ndim + d
            const uint8_t* const raw = (const uint8_t*)a.in;
            const uint64_t tstep = (uint64_t)a.nchan_in * a.npol_in * NDIM;
            if constexpr (NDIM == 2) {
              const uint8_t* const b = raw + (s + n) * tstep + (uint64_t)chan * a.npol_in * 2;
              v0 = make_float2(dec(b[0]), dec(b[1]));
              if (two) v1 = make_float2(dec(b[2]), dec(b[3]));
            } else {
              const uint8_t* const b = raw + (s + 2 * n) * tstep + (uint64_t)chan * a.npol_in;
              v0 = make_float2(dec(b[0]), dec(b[tstep]));
              if (two) v1 = make_float2(dec(b[1]), dec(b[tstep + 1]));
            }
          } else {
            // CASPSR: 4 bytes of polarisation 0, 4 bytes of polarisation 1, repeating; t0 = s + 2 n is even
            const uint64_t t0 = s + 2 * n;
            const uint8_t* const b = (const uint8_t*)a.in + (t0 >> 2) * 8 + (t0 & 3);
            const uint32_t p0 = *(const uint16_t*)b, p1 = *(const uint16_t*)(b + 4);
            v0 = make_float2(dec(p0), dec(p0 >> 8));
            v1 = make_float2(dec(p1), dec(p1 >> 8));
          }
        }
        cx2& d = x[(g2 / 2) * P::R1 + i];
        d.x = (v2f){v0.x, v1.x};
        d.y = (v2f){v0.y, v1.y};
      }
    // staged transform: one plane of C float4 per part, (Re p0, Re p1, Im p0, Im p1) (k_tfp's staging)
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
          // (k comes from the opaque t0: the evaluation stays inside the loop)
          const float c = HOLD_W ? wc[HOLD_W ? j : 0] : wcos(k), sn = HOLD_W ? ws[HOLD_W ? j : 0] : wsin(k);
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

  // the segment's sums, once: this workgroup is the only owner of its slice of the partial array
  uint32_t t0 = threadIdx.x;
  asm volatile("" : "+v"(t0));
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const uint32_t k = t0 + j * nt;
    if (k >= NK) continue;
#pragma unroll
    for (int e = 0; e < NE; e++) {
      const uint32_t bin = e == 0 ? k : (k ? C - k : C / 2);
#pragma unroll
      for (int q = 0; q < NPO; q++)
        a.partial[(((size_t)seg * NPO + q) * a.nchan_in + chan) * C + bin] = acc[j][e][q];
    }
  }
}

// pass[i] += partial[0][i] + partial[1][i] + ... in segment order; n = npol_out * nchan_in * C
__global__ __launch_bounds__(256) void k_bandpass_combine(float* __restrict__ pass, const float* __restrict__ partial,
                                                          const uint32_t nseg, const uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = pass[i];
  for (uint32_t s = 0; s < nseg; s++) v += partial[(uint64_t)s * n + i];
  pass[i] = v;
}

typedef void (*kbp_t)(BpArgs, const cf*);
template <int NDIM, int NPO, int FORM> static kbp_t pick_bp3(const int logc)
{
  static const kbp_t t[] = {nullptr, k_bandpass<1, NDIM, NPO, FORM>, k_bandpass<2, NDIM, NPO, FORM>, k_bandpass<3, NDIM, NPO, FORM>,
                            k_bandpass<4, NDIM, NPO, FORM>, k_bandpass<5, NDIM, NPO, FORM>, k_bandpass<6, NDIM, NPO, FORM>,
                            k_bandpass<7, NDIM, NPO, FORM>, k_bandpass<8, NDIM, NPO, FORM>, k_bandpass<9, NDIM, NPO, FORM>,
                            k_bandpass<10, NDIM, NPO, FORM>, k_bandpass<11, NDIM, NPO, FORM>, k_bandpass<12, NDIM, NPO, FORM>,
                            k_bandpass<13, NDIM, NPO, FORM>};
  return t[logc];
}
template <int NDIM, int FORM> static kbp_t pick_bp2(const int logc, const uint32_t npo)
{
  return npo == 1 ? pick_bp3<NDIM, 1, FORM>(logc) : npo == 2 ? pick_bp3<NDIM, 2, FORM>(logc) : pick_bp3<NDIM, 4, FORM>(logc);
}
static kbp_t pick_bp(const int logc, const uint32_t ndim, const uint32_t npo, const int form)
{
  if (form == BP_CASPSR) return npo == 2 ? pick_bp3<1, 2, BP_CASPSR>(logc) : pick_bp3<1, 4, BP_CASPSR>(logc);   // real, two polarisations
  if (form == BP_GENERIC) return ndim == 2 ? pick_bp2<2, BP_GENERIC>(logc, npo) : pick_bp2<1, BP_GENERIC>(logc, npo);
  return ndim == 2 ? pick_bp2<2, BP_FLOAT>(logc, npo) : pick_bp2<1, BP_FLOAT>(logc, npo);
}

static int bp_fail(char* msg, size_t len, const char* fmt, ...)
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

struct dspsr_amd_bandpass {
  dspsr_amd_ctx* ctx = nullptr;
  uint32_t nchan_in = 0, npol_in = 0, ndim_in = 0, resolution = 0, npol_out = 0;
  uint64_t pass_floats = 0;
  float* pass = nullptr;
  float* partial = nullptr;
  size_t partial_count = 0;
  double integration_samples = 0;
};

extern "C" int dspsr_amd_bandpass_check_shape(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t resolution,
                                              uint32_t npol_out, char* msg, size_t msg_len)
{
  const char* who = "dspsr_amd_bandpass_set_shape";
  if (!resolution)                                          // Bandpass.C:52-54
    return bp_fail(msg, msg_len, "%s: number of output frequency channels == 0 (resolution)", who);
  if (resolution < 2 || resolution > 8192 || (resolution & (resolution - 1)))
    return bp_fail(msg, msg_len, "%s: resolution=%u must be a power of two in [2, 8192]", who, resolution);
  if (ndim_in != 1 && ndim_in != 2)                         // :76-91: detected input is not built
    return bp_fail(msg, msg_len, "%s: ndim_in=%u is neither Nyquist (1) nor Analytic (2); detected input is not built", who, ndim_in);
  if (npol_in != 1 && npol_in != 2) return bp_fail(msg, msg_len, "%s: npol_in=%u not 1 or 2", who, npol_in);
  if (npol_out != npol_in && !(npol_out == 4 && npol_in == 2))              // :66-67, :114-117
    return bp_fail(msg, msg_len, "%s: npol_out=%u must be npol_in=%u, or 4 with npol_in=2", who, npol_out, npol_in);
  if (!nchan_in || nchan_in > 65535)
    return bp_fail(msg, msg_len, "%s: nchan_in=%u outside [1, 65535]", who, nchan_in);
  if (4ull * nchan_in * resolution * sizeof(float) > BP_PARTIAL_BYTES)      // one segment's sums, counted for npol_out = 4
    return bp_fail(msg, msg_len, "%s: nchan_in=%u x resolution=%u > 2^24: the sums of one segment would exceed %llu MiB", who, nchan_in,
                   resolution, (unsigned long long)(BP_PARTIAL_BYTES >> 20));
  return DSPSR_AMD_OK;
}

// the device-free half of accumulate's checks; raw_layout < 0: float rows (strides in floats)
extern "C" int dspsr_amd_bandpass_check_input(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t resolution,
                                              int raw_layout, uint64_t in_addr, uint64_t chan_stride, uint64_t pol_stride,
                                              uint64_t ndat, uint32_t* parts_per_tile, uint32_t* tiles_per_segment,
                                              uint32_t* nsegment, char* msg, size_t msg_len)
{
  const char* who = raw_layout < 0 ? "dspsr_amd_bandpass_accumulate" : "dspsr_amd_bandpass_accumulate_raw";
  if (ndat >= (1ull << 31)) return bp_fail(msg, msg_len, "%s: ndat=%llu >= 2^31", who, (unsigned long long)ndat);
  if (raw_layout < 0) {
    if (in_addr & 3) return bp_fail(msg, msg_len, "%s: rows must be 4-byte aligned (address %#llx)", who, (unsigned long long)in_addr);
    const uint64_t row = ndat * ndim_in;
    if ((npol_in > 1 && pol_stride < row) || (nchan_in > 1 && chan_stride < row))
      return bp_fail(msg, msg_len, "%s: stride shorter than the row of %llu floats", who, (unsigned long long)row);
  } else if (raw_layout == DSPSR_AMD_RAW_UWB16) {
    return bp_fail(msg, msg_len, "%s: raw_layout DSPSR_AMD_RAW_UWB16 (16-bit input) is not built", who);
  } else if (raw_layout == DSPSR_AMD_RAW_CASPSR) {
    if (nchan_in != 1 || npol_in != 2 || ndim_in != 1)
      return bp_fail(msg, msg_len, "%s: DSPSR_AMD_RAW_CASPSR is one channel of two real polarisations (nchan_in=%u npol_in=%u ndim_in=%u)",
                     who, nchan_in, npol_in, ndim_in);
    if (in_addr & 7)
      return bp_fail(msg, msg_len, "%s: a DSPSR_AMD_RAW_CASPSR block starts on an 8-byte group (address %#llx)", who,
                     (unsigned long long)in_addr);
  } else if (raw_layout != DSPSR_AMD_RAW_GENERIC) {
    return bp_fail(msg, msg_len, "%s: unknown raw_layout %d", who, raw_layout);
  }
  const uint64_t nsamp_fft = ndim_in == 2 ? resolution : 2ull * resolution;     // Bandpass.C:78-86
  if (ndat < nsamp_fft)                                                          // :94-96
    return bp_fail(msg, msg_len, "%s: error ndat=%llu < nfft=%llu", who, (unsigned long long)ndat, (unsigned long long)nsamp_fft);
  uint32_t tp, tps, nseg;
  bp_cut((uint32_t)(ndat / nsamp_fft), nchan_in, resolution, tp, tps, nseg);
  if (parts_per_tile) *parts_per_tile = tp;
  if (tiles_per_segment) *tiles_per_segment = tps;
  if (nsegment) *nsegment = nseg;
  return DSPSR_AMD_OK;
}

static void bandpass_release(dspsr_amd_bandpass* f)
{
  (void)hipStreamSynchronize(f->ctx->stream);
  if (f->pass) (void)hipFree(f->pass);
  f->pass = nullptr;
  f->pass_floats = 0;
}

extern "C" int dspsr_amd_bandpass_create(dspsr_amd_ctx* ctx, dspsr_amd_bandpass** out)
{
  if (!ctx || !out) return DSPSR_AMD_EINVAL;
  dspsr_amd_bandpass* f = new dspsr_amd_bandpass;
  f->ctx = ctx;
  *out = f;
  return DSPSR_AMD_OK;
}

extern "C" void dspsr_amd_bandpass_destroy(dspsr_amd_bandpass* f)
{
  if (!f) return;
  bandpass_release(f);
  if (f->partial) (void)hipFree(f->partial);
  delete f;
}

extern "C" int dspsr_amd_bandpass_zero(dspsr_amd_bandpass* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  f->integration_samples = 0;                               // Bandpass::reset_output
  if (!f->pass) return DSPSR_AMD_OK;
  const hipError_t e = hipMemsetAsync(f->pass, 0, f->pass_floats * sizeof(float), f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_bandpass_zero: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_bandpass_set_shape(dspsr_amd_bandpass* f, uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in,
                                            uint32_t resolution, uint32_t npol_out)
{
  if (!f) return DSPSR_AMD_EINVAL;
  char msg[400];
  const int rc = dspsr_amd_bandpass_check_shape(nchan_in, npol_in, ndim_in, resolution, npol_out, msg, sizeof msg);
  if (rc != DSPSR_AMD_OK) return ctx_fail(f->ctx, rc, "%s", msg);
  const bool changed = nchan_in != f->nchan_in || npol_in != f->npol_in || ndim_in != f->ndim_in || resolution != f->resolution ||
                       npol_out != f->npol_out;
  const uint64_t need = (uint64_t)npol_out * nchan_in * resolution;
  if (need != f->pass_floats) {
    bandpass_release(f);
    if (hipMalloc((void**)&f->pass, need * sizeof(float)) != hipSuccess) {
      f->pass = nullptr;
      f->resolution = 0;
      return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_bandpass_set_shape: hipMalloc(%llu floats) failed", (unsigned long long)need);
    }
    f->pass_floats = need;
  }
  f->nchan_in = nchan_in; f->npol_in = npol_in; f->ndim_in = ndim_in; f->resolution = resolution; f->npol_out = npol_out;
  return changed ? dspsr_amd_bandpass_zero(f) : DSPSR_AMD_OK;   // a new shape starts from zero; the same shape keeps its sums
}

static int bandpass_launch(dspsr_amd_bandpass* f, const char* who, const void* in_dev, const int raw_layout, const float scale,
                           const uint64_t chan_stride, const uint64_t pol_stride, const uint64_t ndat)
{
  if (!f->pass) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
  char msg[400];
  uint32_t tp, tps, nseg;
  const int rc = dspsr_amd_bandpass_check_input(f->nchan_in, f->npol_in, f->ndim_in, f->resolution, raw_layout,
                                                (uint64_t)(uintptr_t)in_dev, chan_stride, pol_stride, ndat, &tp, &tps, &nseg, msg,
                                                sizeof msg);
  if (rc != DSPSR_AMD_OK) return ctx_fail(f->ctx, rc, "%s", msg);
  if (!in_dev) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: null input", who);

  int logc = 0;
  while ((1u << logc) < f->resolution) logc++;
  const uint64_t nsamp_fft = f->ndim_in == 2 ? f->resolution : 2ull * f->resolution;
  const uint32_t npart = (uint32_t)(ndat / nsamp_fft);
  const uint64_t n = (uint64_t)f->npol_out * f->nchan_in * f->resolution;
  hipStream_t s = f->ctx->stream;
  if (!grow_device_buffer(s, f->partial, f->partial_count, (size_t)(nseg * n)))
    return ctx_fail(f->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc(%u partial arrays of %llu floats) failed", who, nseg, (unsigned long long)n);

  BpArgs a;
  a.in = in_dev; a.cs = chan_stride; a.ps = pol_stride;
  a.partial = f->partial;
  a.npart = npart; a.pps = tps * tp; a.nchan_in = f->nchan_in; a.npol_in = f->npol_in; a.scale = scale;
  const int form = raw_layout < 0 ? BP_FLOAT : raw_layout == DSPSR_AMD_RAW_CASPSR ? BP_CASPSR : BP_GENERIC;
  const kbp_t k = pick_bp(logc, f->ndim_in, f->npol_out, form);
  const size_t lds = lds_total_words_host(16384, logc) * sizeof(cf);
  hipError_t err = dspsr_amd_allow_lds((const void*)k, lds);
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(err));
  hipLaunchKernelGGL(k, dim3(nseg, f->nchan_in), dim3(BP_THREADS), lds, s, a, f->ctx->tw);
  err = hipGetLastError();
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: launch: %s", who, hipGetErrorString(err));
  hipLaunchKernelGGL(k_bandpass_combine, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, f->pass, (const float*)f->partial, nseg, n);
  err = hipGetLastError();
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: combine launch: %s", who, hipGetErrorString(err));
  f->integration_samples += (double)((uint64_t)npart * nsamp_fft);          // Bandpass.C:164 (the caller divides by the rate)
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_bandpass_accumulate(dspsr_amd_bandpass* f, const float* in_dev, uint64_t chan_stride, uint64_t pol_stride,
                                             uint64_t ndat)
{
  if (!f) return DSPSR_AMD_EINVAL;
  return bandpass_launch(f, "dspsr_amd_bandpass_accumulate", in_dev, -1, 1.f, chan_stride, pol_stride, ndat);
}

extern "C" int dspsr_amd_bandpass_accumulate_raw(dspsr_amd_bandpass* f, const void* raw_dev, int raw_layout, float scale,
                                                 uint64_t ndat)
{
  if (!f) return DSPSR_AMD_EINVAL;
  const char* who = "dspsr_amd_bandpass_accumulate_raw";
  if (raw_layout < 0) return ctx_fail(f->ctx, DSPSR_AMD_EINVAL, "%s: unknown raw_layout %d", who, raw_layout);
  return bandpass_launch(f, who, raw_dev, raw_layout, scale, 0, 0, ndat);
}

extern "C" float* dspsr_amd_bandpass_pass_dev(dspsr_amd_bandpass* f) { return f ? f->pass : nullptr; }

extern "C" int dspsr_amd_bandpass_synch(dspsr_amd_bandpass* f, float* pass_host, double* integration_samples)
{
  if (!f || !pass_host) return DSPSR_AMD_EINVAL;
  if (!f->pass) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "dspsr_amd_bandpass_synch: no shape");
  hipError_t e = hipMemcpyAsync(pass_host, f->pass, f->pass_floats * sizeof(float), hipMemcpyDeviceToHost, f->ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(f->ctx->stream);
  if (e != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "dspsr_amd_bandpass_synch: %s", hipGetErrorString(e));
  if (integration_samples) *integration_samples = f->integration_samples;
  return DSPSR_AMD_OK;
}
