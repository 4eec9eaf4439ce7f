// Passband integration: dsp::Bandpass on the device (the operator behind dspsr -R's RFIFilter and the reference's passband tool).
//
// Semantics: the loop of Signal/General/Bandpass.C:122-162 with Response::integrate (Response.C:456-492, :587-612).  The input of
// every channel is cut into npart = ndat / nsamp_fft whole transforms -- contiguous, not overlapping, part k starts at sample
// k * nsamp_fft; nsamp_fft = 2 * resolution real samples (Nyquist) or resolution complex samples (Analytic); trailing samples
// that do not fill a transform are not read.  Each part is transformed (forward, unnormalised; Nyquist: bins 0 .. resolution - 1
// of the real-to-complex transform, the Nyquist bin dropped), detected -- re * re + im * im per polarisation, or PP, QQ, Re P* Q,
// Im P* Q (cross_detect_int) -- and added to pass[npol_out][nchan_in][resolution].
//
// The tile -- C = resolution complex points x the (part, polarisation) columns of Tp = 8192 / C parts, its staged transform, the
// Hermitian split of Nyquist rows, detection and the register sums of the bins a thread owns -- is spectral_tile.h's, shared with
// k_plfb.  Here: no window list; three input forms (float rows, the 8-bit block in the generic order, the 8-bit block in the CASPSR
// order, decoded as k_tfp decodes them: value = (int8 + 0.5) * scale); and one destination only.
//
// Accumulation: the parts of a call are cut into SEGMENTS of whole tiles.  Workgroup (segment, input channel) keeps its sums in
// registers over all tiles of its segment, in time order, and stores them once to partial[segment][npol_out][chan][C];
// k_bandpass_combine -- one owner per element -- adds the partial arrays to the passband in segment order.  The cut depends on
// (npart, nchan_in, resolution) alone and there are no atomics: the same calls give the same bits.
#include "engine_internal.h"
#include "spectral_tile.h"

namespace dspsr_amd {

// The partial arrays of a launch take at most SEG_BYTES, counted for npol_out = 4 (set_shape refuses a shape whose ONE partial array
// would exceed it).

enum { BP_FLOAT = 0, BP_GENERIC = 1, BP_CASPSR = 2 };

struct BpArgs {
  const void* in;                 // float rows: element (chan, pol, t) = in + chan * cs + pol * ps + t * ndim; or the 8-bit block
  uint64_t cs, ps;
  float* partial;                 // [segment][npol_out][nchan_in][C]
  uint32_t npart, pps;            // parts of the call; parts per segment (a multiple of the tile's)
  uint32_t nchan_in, npol_in;
  float scale;
};

template <int LOGC, int NDIM, int NPO, int FORM>
__global__ __launch_bounds__(ST_THREADS) void k_bandpass(const BpArgs a, const cf* __restrict__ tw)
{
  // NPO == 1: p0 alone, npol_out == npol_in.  The Nyquist twiddles are held in registers where a thread owns at most 4 bin pairs;
  // with 8 (C = 8192: one part per tile) the 16 registers go to the sums instead and the two values are evaluated per use
  typedef SpectralTile<LOGC, NDIM, NPO, false, 4> T;
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  uint32_t tid = threadIdx.x;
  constexpr uint32_t NSAMP = NDIM == 2 ? T::C : 2 * T::C;   // samples of a part
  const uint32_t ltw_off = T::fill_twiddle_table(lds, tw, tid);
  const uint32_t chan = blockIdx.y, seg = blockIdx.x;
  const uint32_t w_begin = seg * a.pps, w_end = min(w_begin + a.pps, a.npart);
  const bool two = a.npol_in > 1;                           // one input polarisation: the second column of every pair is zero
  const float hs = 0.5f * a.scale;

  typename T::Tw wc, ws;
  T::twiddles(wc, ws);
  typename T::Acc acc;
  T::zero(acc);

  auto dec = [&](const uint32_t b) { return __builtin_fmaf((float)(int8_t)(b & 0xff), a.scale, hs); };
  auto load = [&](const uint32_t w, const uint32_t n, float2& v0, float2& v1) {
    const uint64_t s = (uint64_t)w * NSAMP;                 // part w starts here: no window list
    if constexpr (FORM == BP_FLOAT) {
      const float* const row0 = (const float*)a.in + chan * a.cs;
      const float* const row1 = row0 + a.ps;
      const uint64_t o = (s << (NDIM - 1)) + 2 * n;         // any float address: two 4-byte loads
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
  };

  for (uint32_t w0 = w_begin; w0 < w_end; w0 += T::Tp) {
    T::transform(lds, ltw_off, tid, w0, w_end, load);
    const uint32_t nw = min(T::Tp, w_end - w0);
    for (uint32_t c2 = 0; c2 < nw; c2++) T::add_part(acc, lds, c2, wc, ws);
    __syncthreads();                                        // the next tile's exchanges overwrite the staged image
  }

  // the segment's sums, once: this workgroup is the only owner of its slice of the partial array
  T::for_owned([&](const int j, const int e, const uint32_t bin) {
#pragma unroll
    for (int q = 0; q < NPO; q++)
      a.partial[(((size_t)seg * NPO + q) * a.nchan_in + chan) * T::C + bin] = acc[j][e][q];
  });
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

}  // namespace dspsr_amd
using namespace dspsr_amd;

struct dspsr_amd_bandpass {
  dspsr_amd_ctx* ctx = nullptr;
  uint32_t nchan_in = 0, npol_in = 0, ndim_in = 0, resolution = 0, npol_out = 0;
  device_sums pass;               // [npol_out][nchan_in][resolution]
  float* partial = nullptr;
  size_t partial_count = 0;
  double integration_samples = 0;
};

extern "C" int dspsr_amd_bandpass_check_shape(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t resolution,
                                              uint32_t npol_out, char* msg, size_t msg_len)
{
  const char* who = "dspsr_amd_bandpass_set_shape";
  if (!resolution)                                          // Bandpass.C:52-54
    return msg_fail(msg, msg_len, "%s: number of output frequency channels == 0 (resolution)", who);
  if (resolution < 2 || resolution > 8192 || (resolution & (resolution - 1)))
    return msg_fail(msg, msg_len, "%s: resolution=%u must be a power of two in [2, 8192]", who, resolution);
  if (ndim_in != 1 && ndim_in != 2)                         // :76-91: detected input is not built
    return msg_fail(msg, msg_len, "%s: ndim_in=%u is neither Nyquist (1) nor Analytic (2); detected input is not built", who, ndim_in);
  if (npol_in != 1 && npol_in != 2) return msg_fail(msg, msg_len, "%s: npol_in=%u not 1 or 2", who, npol_in);
  if (npol_out != npol_in && !(npol_out == 4 && npol_in == 2))              // :66-67, :114-117
    return msg_fail(msg, msg_len, "%s: npol_out=%u must be npol_in=%u, or 4 with npol_in=2", who, npol_out, npol_in);
  if (!nchan_in || nchan_in > 65535)
    return msg_fail(msg, msg_len, "%s: nchan_in=%u outside [1, 65535]", who, nchan_in);
  if (4ull * nchan_in * resolution * sizeof(float) > SEG_BYTES)      // one segment's sums, counted for npol_out = 4
    return msg_fail(msg, msg_len, "%s: nchan_in=%u x resolution=%u > 2^24: the sums of one segment would exceed %llu MiB", who, nchan_in,
                    resolution, (unsigned long long)(SEG_BYTES >> 20));
  return DSPSR_AMD_OK;
}

// the device-free half of accumulate's checks; raw_layout < 0: float rows (strides in floats)
extern "C" int dspsr_amd_bandpass_check_input(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t resolution,
                                              int raw_layout, uint64_t in_addr, uint64_t chan_stride, uint64_t pol_stride,
                                              uint64_t ndat, uint32_t* parts_per_tile, uint32_t* tiles_per_segment,
                                              uint32_t* nsegment, char* msg, size_t msg_len)
{
  const char* who = raw_layout < 0 ? "dspsr_amd_bandpass_accumulate" : "dspsr_amd_bandpass_accumulate_raw";
  if (ndat >= (1ull << 31)) return msg_fail(msg, msg_len, "%s: ndat=%llu >= 2^31", who, (unsigned long long)ndat);
  if (raw_layout < 0) {
    if (in_addr & 3) return msg_fail(msg, msg_len, "%s: rows must be 4-byte aligned (address %#llx)", who, (unsigned long long)in_addr);
    const uint64_t row = ndat * ndim_in;
    if ((npol_in > 1 && pol_stride < row) || (nchan_in > 1 && chan_stride < row))
      return msg_fail(msg, msg_len, "%s: stride shorter than the row of %llu floats", who, (unsigned long long)row);
  } else if (raw_layout == DSPSR_AMD_RAW_UWB16) {
    return msg_fail(msg, msg_len, "%s: raw_layout DSPSR_AMD_RAW_UWB16 (16-bit input) is not built", who);
  } else if (raw_layout == DSPSR_AMD_RAW_CASPSR) {
    if (nchan_in != 1 || npol_in != 2 || ndim_in != 1)
      return msg_fail(msg, msg_len, "%s: DSPSR_AMD_RAW_CASPSR is one channel of two real polarisations (nchan_in=%u npol_in=%u ndim_in=%u)",
                      who, nchan_in, npol_in, ndim_in);
    if (in_addr & 7)
      return msg_fail(msg, msg_len, "%s: a DSPSR_AMD_RAW_CASPSR block starts on an 8-byte group (address %#llx)", who,
                      (unsigned long long)in_addr);
  } else if (raw_layout != DSPSR_AMD_RAW_GENERIC) {
    return msg_fail(msg, msg_len, "%s: unknown raw_layout %d", who, raw_layout);
  }
  const uint64_t nsamp_fft = ndim_in == 2 ? resolution : 2ull * resolution;     // Bandpass.C:78-86
  if (ndat < nsamp_fft)                                                          // :94-96
    return msg_fail(msg, msg_len, "%s: error ndat=%llu < nfft=%llu", who, (unsigned long long)ndat, (unsigned long long)nsamp_fft);
  // the launch arithmetic (pure; tests/bandpass_cases.py restates it): parts per tile, tiles per segment, segments
  const uint32_t tp = 8192u / resolution, npart = (uint32_t)(ndat / nsamp_fft);
  uint32_t tps, nseg;
  segment_cut((npart + tp - 1) / tp, nchan_in, SEG_BYTES / (4ull * nchan_in * resolution * sizeof(float)), tps, nseg);
  if (parts_per_tile) *parts_per_tile = tp;
  if (tiles_per_segment) *tiles_per_segment = tps;
  if (nsegment) *nsegment = nseg;
  return DSPSR_AMD_OK;
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
  sums_release(f->ctx, f->pass);
  if (f->partial) (void)hipFree(f->partial);
  delete f;
}

extern "C" int dspsr_amd_bandpass_zero(dspsr_amd_bandpass* f)
{
  if (!f) return DSPSR_AMD_EINVAL;
  f->integration_samples = 0;                               // Bandpass::reset_output
  return sums_zero(f->ctx, f->pass, "dspsr_amd_bandpass_zero");
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
  if (sums_resize(f->ctx, f->pass, (uint64_t)npol_out * nchan_in * resolution, "dspsr_amd_bandpass_set_shape") != DSPSR_AMD_OK) {
    f->resolution = 0;
    return DSPSR_AMD_ENOMEM;
  }
  f->nchan_in = nchan_in; f->npol_in = npol_in; f->ndim_in = ndim_in; f->resolution = resolution; f->npol_out = npol_out;
  return changed ? dspsr_amd_bandpass_zero(f) : DSPSR_AMD_OK;   // a new shape starts from zero; the same shape keeps its sums
}

static int bandpass_launch(dspsr_amd_bandpass* f, const char* who, const void* in_dev, const int raw_layout, const float scale,
                           const uint64_t chan_stride, const uint64_t pol_stride, const uint64_t ndat)
{
  if (!f->pass.dev) return ctx_fail(f->ctx, DSPSR_AMD_ESTATE, "%s: no shape", who);
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
  hipLaunchKernelGGL(k, dim3(nseg, f->nchan_in), dim3(ST_THREADS), lds, s, a, f->ctx->tw);
  err = hipGetLastError();
  if (err != hipSuccess) return ctx_fail(f->ctx, DSPSR_AMD_EHIP, "%s: launch: %s", who, hipGetErrorString(err));
  hipLaunchKernelGGL(k_bandpass_combine, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, f->pass.dev, (const float*)f->partial, nseg, n);
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

extern "C" float* dspsr_amd_bandpass_pass_dev(dspsr_amd_bandpass* f) { return f ? f->pass.dev : nullptr; }

extern "C" int dspsr_amd_bandpass_synch(dspsr_amd_bandpass* f, float* pass_host, double* integration_samples)
{
  if (!f || !pass_host) return DSPSR_AMD_EINVAL;
  const int rc = sums_synch(f->ctx, f->pass, pass_host, "dspsr_amd_bandpass_synch");
  if (rc != DSPSR_AMD_OK) return rc;
  if (integration_samples) *integration_samples = f->integration_samples;
  return DSPSR_AMD_OK;
}
