// Search mode on already channelised 8-bit voltages, `digifil file.dada` with no -F (Signal/General/LoadToFil.C:233-304):
//   k_unpack_fpt   the generic 8-bit unpacker (Kernel/Classes/BitUnpacker.C:48-80; CUDA twin GenericEightBitUnpackerCUDA.cu:24-83,
//                  which walks the block with a stride of a whole time sample between lanes): raw TFP block -> float FPT rows
//   k_detect_raw   unpack -> Detection::square_law / polarimetry (Detection.C:218-320, LoadToFil.C:262-277) -> TScrunch, FPT
//                  branch (TScrunch.C:148-178) in ONE pass: the float voltage rows never exist in memory (4 B per dual-pol
//                  (channel, sample) read instead of 4 B read + 16 B written + 16 B read)
// Byte order of the block: ((t * nchan + c) * npol + p) * ndim + d, two's-complement int8, value (float(s) + 0.5f) * scale.
// Both kernels read along the bytes of a time sample and turn the tile through LDS, so that every output row is written in
// contiguous runs along time.
#include "engine_internal.h"

namespace dspsr_amd {

// the decoded sample, formed in one place: k_detect_raw must see the floats k_unpack_fpt writes
__device__ __forceinline__ float raw8(const int s, const float scale)
{
  const float v = (float)s + 0.5f;
  return v * scale;
}
__device__ __forceinline__ int byte_of(const uint32_t w, const int k) { return (int)(int8_t)(w >> (8 * k)); }

struct __attribute__((packed, aligned(4))) raw_w4 { uint32_t w[4]; };     // 16 bytes at a 4-byte aligned address
struct __attribute__((packed, aligned(4))) raw_w2 { uint32_t w[2]; };

// ---- k_unpack_fpt ------------------------------------------------------------------------------------------------------------
// A tile = tt time samples x up to 64 bytes of the (chan, pol, dim) axis; tt = 64 when a time sample has >= 64 bytes, more when it
// is narrower (4096 bytes of the block per tile either way).  LDS row = one output row (chan, pol) of the tile, tt * ndim floats +
// ndim floats of padding: the lanes of a load run along the bytes of a sample = down the LDS rows, row stride = ndim (mod 32) banks.
#define UNPACK_TW 64
#define UNPACK_LDS (4096 + 64)
template <bool WORDS>
__global__ __launch_bounds__(256) void k_unpack_fpt(const int8_t* __restrict__ raw, const float scale, const uint32_t width /* bytes per time sample */,
                                                    const uint32_t npol, const uint32_t ndim, const uint64_t ndat, float* __restrict__ out,
                                                    const uint64_t ocs, const uint64_t ops, const uint32_t tt, const uint32_t nwt, const uint64_t ntile)
{
  __shared__ float lds[UNPACK_LDS];
  const uint32_t cols = tt * ndim, S = cols + ndim;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t t0 = (tile / nwt) * tt;
    const uint32_t w0 = (uint32_t)(tile % nwt) * UNPACK_TW;
    const uint32_t tw = width - w0 < UNPACK_TW ? width - w0 : UNPACK_TW;
    const uint32_t nt = ndat - t0 < tt ? (uint32_t)(ndat - t0) : tt;
    if (WORDS) {                                          // raw, width and tw are multiples of 4: one aligned word per lane
      const uint32_t wq = tw / 4;
      for (uint32_t e = threadIdx.x; e < nt * wq; e += 256) {
        const uint32_t t = e / wq, w = (e - t * wq) * 4;
        const uint32_t v = *(const uint32_t*)(raw + (t0 + t) * width + w0 + w);
  #pragma unroll
        for (int k = 0; k < 4; k++) lds[((w + k) / ndim) * S + t * ndim + (w + k) % ndim] = raw8(byte_of(v, k), scale);
      }
    } else {
      for (uint32_t e = threadIdx.x; e < nt * tw; e += 256) {
        const uint32_t t = e / tw, w = e - t * tw;
        lds[(w / ndim) * S + t * ndim + w % ndim] = raw8((int)raw[(t0 + t) * width + w0 + w], scale);
      }
    }
    __syncthreads();
    const uint32_t rows = tw / ndim, ncol = nt * ndim;
    for (uint32_t e = threadIdx.x; e < rows * cols; e += 256) {
      const uint32_t r = e / cols, col = e - r * cols;     // (cols is a power of two)
      if (col < ncol) {
        const uint32_t row = w0 / ndim + r;
        out[(uint64_t)(row / npol) * ocs + (uint64_t)(row % npol) * ops + t0 * ndim + col] = lds[r * S + col];
      }
    }
    __syncthreads();
  }
}

// ---- k_detect_raw ------------------------------------------------------------------------------------------------------------
// 256 threads = LC lanes along the channels (VEC channels each: 16 bytes of a dual-pol sample with VEC 4) x LT = 256 / LC lanes
// along time; LC = 64 for wide bands, smaller for few channels, so that a wave spreads over time instead of idling.  A thread sums
// the tscrunch consecutive samples of one output sample in registers, G output samples per tile (o = i * LT + lt), and the tile of
// LC * VEC channels x NOUT products x OT = LT * G outputs is turned through LDS: a store runs along the time axis of one row.
//   LDS row = (v * NOUT + r) * LC + lc, row stride OT + max(1, 32 / LC) floats: the 32 lanes of a half wave (lc fastest, then lt)
//   write to 32 different banks (OT is a multiple of 32 when LC < 32 and even otherwise); the reads run along a row.
// The stream contract is that of dspsr_amd_filterbank_perform_search.  Output sample 0 starts from the carry when c0 > 0; the open
// group behind the last complete output replaces the carry and belongs to the SAME thread, after its read (k_tscrunch_fpt, scrunch.hip).
template <int NPOL, int STATE> struct detect_shape {
  static constexpr int NOUT = STATE == DSPSR_AMD_COHERENCE ? 4 : STATE == DSPSR_AMD_PPQQ ? 2 : 1;
};
#define DETECT_RAW_LDS (8192 + 1024)

// the NOUT products of one (channel, sample): w = the 2 * NPOL bytes of the channel
template <int NPOL, int STATE>
__device__ __forceinline__ void detect_one(const uint32_t w, const float scale, float* v)
{
  const float2 a = make_float2(raw8(byte_of(w, 0), scale), raw8(byte_of(w, 1), scale));
  if (NPOL == 1) {
    v[0] = __fadd_rn(__fmul_rn(a.x, a.x), __fmul_rn(a.y, a.y));                    // k_square_law (detect.hip)
    return;
  }
  const float2 b = make_float2(raw8(byte_of(w, 2), scale), raw8(byte_of(w, 3), scale));
  if (STATE == DSPSR_AMD_COHERENCE) {                                              // k_polarimetry (detect.hip), ndim 1
    const float pp = a.x * a.x + a.y * a.y;
    const float qq = b.x * b.x + b.y * b.y;
    const float re = a.x * b.x + a.y * b.y;
    const float im = a.x * b.y - a.y * b.x;
    v[0] = pp; v[1] = qq; v[2] = re; v[3] = im;
  } else {
    const float p = __fadd_rn(__fmul_rn(a.x, a.x), __fmul_rn(a.y, a.y));
    const float q = __fadd_rn(__fmul_rn(b.x, b.x), __fmul_rn(b.y, b.y));
    if (STATE == DSPSR_AMD_INTENSITY) v[0] = __fadd_rn(p, q);                      // Detection.C:285-300: *p0 += *p1
    else { v[0] = p; v[1] = q; }
  }
}

// the bytes of VEC consecutive channels of one time sample, one 32-bit word per channel (NPOL 1: the low 16 bits)
template <int NPOL, int VEC>
__device__ __forceinline__ void load_chans(const int8_t* __restrict__ p, const uint32_t nvalid, uint32_t* w)
{
  if (VEC == 4 && nvalid == 4) {                             // (the host takes VEC 4 only where these addresses are 4-byte aligned)
    if (NPOL == 2) {
      const raw_w4 x = *(const raw_w4*)p;
  #pragma unroll
      for (int v = 0; v < 4; v++) w[v] = x.w[v];
    } else {
      const raw_w2 x = *(const raw_w2*)p;
      w[0] = x.w[0] & 0xffffu; w[1] = x.w[0] >> 16; w[2] = x.w[1] & 0xffffu; w[3] = x.w[1] >> 16;
    }
    return;
  }
  #pragma unroll
  for (int v = 0; v < VEC; v++) {
    w[v] = 0;
    if ((uint32_t)v < nvalid) {
      const int8_t* q = p + v * 2 * NPOL;
      if (NPOL == 2 && ((uintptr_t)q & 3) == 0) w[v] = *(const uint32_t*)q;
      else {
  #pragma unroll
        for (int k = 0; k < 2 * NPOL; k++) w[v] |= (uint32_t)(uint8_t)q[k] << (8 * k);
      }
    }
  }
}

// stream samples [s0, s1) of VEC channels summed in time order; from_carry: acc already holds the samples in front of them
template <int NPOL, int STATE, int VEC>
__device__ __forceinline__ void sum_group(const int8_t* __restrict__ raw, const float scale, const uint64_t sample_bytes, const uint32_t nvalid,
                                          uint64_t i, const uint64_t i1, bool have, float (*acc)[detect_shape<NPOL, STATE>::NOUT])
{
  constexpr int NOUT = detect_shape<NPOL, STATE>::NOUT;
  #pragma unroll 4
  for (; i < i1; i++) {
    uint32_t w[VEC];
    load_chans<NPOL, VEC>(raw + i * sample_bytes, nvalid, w);
  #pragma unroll
    for (int v = 0; v < VEC; v++) {
      float d[NOUT];
      detect_one<NPOL, STATE>(w[v], scale, d);
  #pragma unroll
      for (int r = 0; r < NOUT; r++) acc[v][r] = have ? __fadd_rn(acc[v][r], d[r]) : d[r];     // out = in[0]; out += in[1]; ...
    }
    have = true;
  }
}

template <int NPOL, int STATE, int VEC>
__global__ __launch_bounds__(256) void k_detect_raw(const int8_t* __restrict__ raw, const float scale, const uint32_t nchan, const uint64_t ndat,
                                                    const uint32_t ts, const uint32_t c0, float* __restrict__ out, const uint64_t ocs,
                                                    const uint64_t ops, float* carry, const uint64_t nout, const uint32_t rem,
                                                    const uint32_t lc_log2, const uint32_t nctile, const uint64_t ntile)
{
  constexpr int NOUT = detect_shape<NPOL, STATE>::NOUT;
  constexpr int G = 32 / (VEC * NOUT) < 8 ? 32 / (VEC * NOUT) : 8;
  __shared__ float lds[DETECT_RAW_LDS];
  const uint32_t LC = 1u << lc_log2, LT = 256u >> lc_log2, OT = LT * G, S = OT + (LC < 32 ? 32 / LC : 1);
  const uint32_t lc = threadIdx.x & (LC - 1), lt = threadIdx.x >> lc_log2;
  const uint64_t sample_bytes = (uint64_t)nchan * NPOL * 2;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint32_t ch0 = (uint32_t)(tile % nctile) * LC * VEC;
    const uint64_t o0 = (tile / nctile) * OT;
    const uint32_t ch = ch0 + lc * VEC;
    const uint32_t nvalid = ch >= nchan ? 0 : nchan - ch < VEC ? nchan - ch : VEC;
    const int8_t* __restrict__ p = raw + (uint64_t)ch * NPOL * 2;
    if (nvalid) {
  #pragma unroll
      for (int i = 0; i < G; i++) {
        const uint64_t o = o0 + (uint32_t)i * LT + lt;
        float acc[VEC][NOUT];
  #pragma unroll
        for (int v = 0; v < VEC; v++)
  #pragma unroll
          for (int r = 0; r < NOUT; r++) acc[v][r] = 0.f;
        if (o < nout) {
          // stream samples [o*ts, (o+1)*ts) = input samples [o*ts - c0, ...)
          const uint64_t s0 = o * ts;
          const bool first = o == 0 && c0;
          if (first)
  #pragma unroll
            for (int v = 0; v < VEC; v++)
  #pragma unroll
              for (int r = 0; r < NOUT; r++)
                if ((uint32_t)v < nvalid) acc[v][r] = carry[(uint64_t)(ch + v) * NOUT + r];
          sum_group<NPOL, STATE, VEC>(p, scale, sample_bytes, nvalid, s0 < c0 ? 0 : s0 - c0, s0 + ts - c0, first, acc);
  #pragma unroll
          for (int v = 0; v < VEC; v++)
  #pragma unroll
            for (int r = 0; r < NOUT; r++) lds[((v * NOUT + r) * LC + lc) * S + (uint32_t)i * LT + lt] = acc[v][r];
        }
        if (o == 0 && rem) {
          // the open group: stream samples [nout*ts, nout*ts + rem); it starts from the carry when no output was completed.  This
          // thread has read the old carry above (nout > 0) or reads it here: nobody else touches these carry elements.
          const uint64_t s0 = nout * ts;
          const bool first = nout == 0 && c0;
          if (first)
  #pragma unroll
            for (int v = 0; v < VEC; v++)
  #pragma unroll
              for (int r = 0; r < NOUT; r++)
                if ((uint32_t)v < nvalid) acc[v][r] = carry[(uint64_t)(ch + v) * NOUT + r];
          sum_group<NPOL, STATE, VEC>(p, scale, sample_bytes, nvalid, s0 < c0 ? 0 : s0 - c0, s0 + rem - c0, first, acc);
  #pragma unroll
          for (int v = 0; v < VEC; v++)
  #pragma unroll
            for (int r = 0; r < NOUT; r++)
              if ((uint32_t)v < nvalid) carry[(uint64_t)(ch + v) * NOUT + r] = acc[v][r];
        }
      }
    }
    __syncthreads();
    // rows of the tile -> rows of the output, lanes along time
    const uint32_t ot_log2 = 31 - __clz(OT);
    for (uint32_t e = threadIdx.x; e < VEC * NOUT * LC * OT; e += 256) {
      const uint32_t row = e >> ot_log2, col = e & (OT - 1);
      const uint32_t vr = row >> lc_log2, c = ch0 + (row & (LC - 1)) * VEC + vr / NOUT, r = vr % NOUT;
      if (c < nchan && o0 + col < nout) out[(uint64_t)c * ocs + (uint64_t)r * ops + o0 + col] = lds[row * S + col];
    }
    __syncthreads();
  }
}

template <int NPOL, int STATE, int VEC>
static void launch_detect_raw(hipStream_t stream, uint32_t ncu, const int8_t* raw, float scale, uint32_t nchan, uint64_t ndat, uint32_t ts, uint32_t c0,
                              float* out, uint64_t ocs, uint64_t ops, float* carry, uint64_t nout, uint32_t rem)
{
  constexpr int NOUT = detect_shape<NPOL, STATE>::NOUT;
  constexpr int G = 32 / (VEC * NOUT) < 8 ? 32 / (VEC * NOUT) : 8;
  const uint32_t nlane = (nchan + VEC - 1) / VEC;
  uint32_t lc_log2 = 0;
  while (lc_log2 < 6 && (1u << lc_log2) < nlane) lc_log2++;
  const uint32_t LC = 1u << lc_log2, OT = (256u >> lc_log2) * G;
  const uint32_t nctile = (nlane + LC - 1) / LC;
  const uint64_t nown = nout ? nout : 1;                                  // (nout == 0: the open group alone, with output 0's thread)
  const uint64_t ntile = (uint64_t)nctile * ((nown + OT - 1) / OT);
  const uint64_t cap = (uint64_t)(ncu ? ncu : 256) * 32;
  hipLaunchKernelGGL((k_detect_raw<NPOL, STATE, VEC>), dim3((uint32_t)(ntile < cap ? ntile : cap)), dim3(256), 0, stream, raw, scale, nchan, ndat, ts,
                     c0, out, ocs, ops, carry, nout, rem, lc_log2, nctile, ntile);
}

}  // namespace dspsr_amd

using namespace dspsr_amd;

extern "C" int dspsr_amd_unpack_fpt(dspsr_amd_ctx* ctx, const int8_t* raw_dev, float scale, uint32_t nchan, uint32_t npol, uint32_t ndim,
                                    uint64_t ndat, float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride)
{
  if (!ctx) return DSPSR_AMD_EINVAL;
  if (!nchan || (npol != 1 && npol != 2 && npol != 4) || (ndim != 1 && ndim != 2))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_fpt: nchan=%u npol=%u ndim=%u (nchan >= 1, npol 1 / 2 / 4, ndim 1 / 2)", nchan, npol, ndim);
  const uint64_t width64 = (uint64_t)nchan * npol * ndim;
  if (width64 > 0x7fffffffull) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_fpt: nchan=%u is too large", nchan);
  if (!ndat) return DSPSR_AMD_OK;
  if (!raw_dev || !out_dev) return DSPSR_AMD_EINVAL;
  const uint64_t nfloat = ndat * ndim;
  if ((npol > 1 && out_pol_stride < nfloat) || (nchan > 1 && out_chan_stride < (npol - 1) * out_pol_stride + nfloat))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_unpack_fpt: output rows of %llu floats overlap (chan stride %llu, pol stride %llu)",
                    (unsigned long long)nfloat, (unsigned long long)out_chan_stride, (unsigned long long)out_pol_stride);
  const uint32_t width = (uint32_t)width64;
  uint32_t p2 = 1;
  while (p2 < width && p2 < UNPACK_TW) p2 <<= 1;
  const uint32_t tt = 64 * (UNPACK_TW / p2), nwt = (width + UNPACK_TW - 1) / UNPACK_TW;
  const uint64_t ntile = (uint64_t)nwt * ((ndat + tt - 1) / tt);
  const uint64_t cap = (uint64_t)(ctx->ncu ? ctx->ncu : 256) * 32;
  const dim3 grid((uint32_t)(ntile < cap ? ntile : cap));
  if (((uintptr_t)raw_dev % 4) == 0 && (width % 4) == 0)                // (then every 64-byte tile of a sample is whole words too)
    hipLaunchKernelGGL(k_unpack_fpt<true>, grid, dim3(256), 0, ctx->stream, raw_dev, scale, width, npol, ndim, ndat, out_dev, out_chan_stride,
                       out_pol_stride, tt, nwt, ntile);
  else
    hipLaunchKernelGGL(k_unpack_fpt<false>, grid, dim3(256), 0, ctx->stream, raw_dev, scale, width, npol, ndim, ndat, out_dev, out_chan_stride,
                       out_pol_stride, tt, nwt, ntile);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_unpack_fpt: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_detect_raw(dspsr_amd_ctx* ctx, const int8_t* raw_dev, float scale, uint32_t nchan, uint32_t npol, uint64_t ndat,
                                    int out_state, uint32_t tscrunch, float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride,
                                    float* carry_dev, uint32_t* carry_count, uint64_t* nout)
{
  if (!ctx || !nout) return DSPSR_AMD_EINVAL;
  if (!nchan || (npol != 1 && npol != 2))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_detect_raw: nchan=%u npol=%u (nchan >= 1, npol 1 / 2)", nchan, npol);
  if (out_state != DSPSR_AMD_INTENSITY && out_state != DSPSR_AMD_PPQQ && out_state != DSPSR_AMD_COHERENCE)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_detect_raw: invalid state=%d", out_state);
  if (npol == 1 && out_state != DSPSR_AMD_INTENSITY)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_detect_raw: state=%d needs two input polarisations", out_state);
  if (!tscrunch) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dsp::TScrunch::get_factor scrunch factor not set");       // TScrunch.C:88-90
  if (tscrunch > 1 && (!carry_dev || !carry_count))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_detect_raw: tscrunch=%u needs carry_dev and carry_count", tscrunch);
  const uint32_t c0 = carry_count ? *carry_count : 0;
  if (c0 >= tscrunch)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_detect_raw: carry_count=%u must be < tscrunch=%u", c0, tscrunch);
  if ((uint64_t)nchan * 4 > 0x7fffffffull) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_detect_raw: nchan=%u is too large", nchan);
  const uint64_t total = (uint64_t)c0 + ndat, no = total / tscrunch;
  const uint32_t rem = (uint32_t)(total % tscrunch);
  if (!ndat) { *nout = no; return DSPSR_AMD_OK; }                        // (no = 0: c0 < tscrunch)
  if (!raw_dev || (!out_dev && no)) return DSPSR_AMD_EINVAL;
  const uint32_t npo = out_state == DSPSR_AMD_COHERENCE ? 4 : out_state == DSPSR_AMD_PPQQ ? 2 : 1;
  if (no && ((npo > 1 && out_pol_stride < no) || (nchan > 1 && out_chan_stride < (npo - 1) * out_pol_stride + no)))
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_detect_raw: output rows of %llu floats overlap (chan stride %llu, pol stride %llu)",
                    (unsigned long long)no, (unsigned long long)out_chan_stride, (unsigned long long)out_pol_stride);
  // four channels per lane where their bytes start on a 4-byte boundary in every time sample
  const bool vec = nchan >= 4 && ((uintptr_t)raw_dev % 4) == 0 && (npol == 2 || (nchan % 2) == 0);
  #define DETECT_RAW_GO(NPOL, STATE)                                                                                                            \
    do {                                                                                                                                        \
      if (vec) launch_detect_raw<NPOL, STATE, 4>(ctx->stream, ctx->ncu, raw_dev, scale, nchan, ndat, tscrunch, c0, out_dev, out_chan_stride,   \
                                                 out_pol_stride, carry_dev, no, rem);                                                          \
      else launch_detect_raw<NPOL, STATE, 1>(ctx->stream, ctx->ncu, raw_dev, scale, nchan, ndat, tscrunch, c0, out_dev, out_chan_stride,       \
                                             out_pol_stride, carry_dev, no, rem);                                                              \
    } while (0)
  if (npol == 1) DETECT_RAW_GO(1, DSPSR_AMD_INTENSITY);
  else if (out_state == DSPSR_AMD_INTENSITY) DETECT_RAW_GO(2, DSPSR_AMD_INTENSITY);
  else if (out_state == DSPSR_AMD_PPQQ) DETECT_RAW_GO(2, DSPSR_AMD_PPQQ);
  else DETECT_RAW_GO(2, DSPSR_AMD_COHERENCE);
  #undef DETECT_RAW_GO
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_detect_raw: %s", hipGetErrorString(e));
  if (carry_count) *carry_count = rem;                                   // (only once the launch is in, as dspsr_amd_tscrunch_fpt)
  *nout = no;
  return DSPSR_AMD_OK;
}
