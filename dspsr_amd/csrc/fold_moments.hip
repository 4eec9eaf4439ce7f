// Fourth-order moments of the Stokes parameters, `dspsr -4` (LoadToFold1.C:552-568,1119-1123), for gfx950.
// Reference: dsp::FourthMoment::transformation (Signal/General/FourthMoment.C:29-77: Stokes ndim 4 in, npol 1 x ndim 14 out --
// the four Stokes parameters, then in[i] * in[j] for i <= j in the order 00 01 02 03 11 12 13 22 23 33), folded by the plain sum
// of Fold.C:835-891 over the 14 floats of every sample; the Archiver turns the folded moments into covariances
// (Archiver.C:679-713,738-771; host side: pipeline.moments_to_central).
//
//   k_fourth_moment   the stand-alone operation: rows of ndat*4 floats in, rows of ndat*14 floats out, out of place.
//   k_fold_moments    Fold::Engine::fold into a profile of npol 1 x ndim 14, with two loaders over ONE accumulation body:
//     STOKES   reads the ndim 4 rows and forms the ten products in registers (one rounded multiply each, never contracted
//              into the add): the 56-byte stream -- 3.5 times the detected bytes, written once and read once -- never exists;
//     stream   reads ndim 14 rows as they are (the Fold::Engine surface: its input is the output of a FourthMoment operation).
//   Both give the same bits on the same Stokes samples: every (chan, bin, component) sum has one association, below.
//
// The contract of fold.hip holds: no atomics, one owner thread per (chan, bin) accumulator, the same bits run to run.
//   exact  (every run of the plan shorter than FOLD_LONG_RUN)  the owner starts from the profile and adds the bin's samples one by
//          one in time order: the association of Fold.C:844-852, whatever the chunk size, bin split or alignment.
//   LONG   (a run of FOLD_LONG_RUN samples or more)  as k_fold_chunked<., true, .>: the row is cut into time segments of
//          `seg_samples` samples counted from `first` (a multiple of MOM_SEG_UNIT, so both loaders' chunk grids nest in it); a
//          segment is summed from zero -- per run piece: single samples up to the first MOM_MB boundary (counted from `first`)
//          inside the piece, whole micro-block sums (each summed from zero in time order), single samples behind the last
//          boundary -- into its partial profile, and k_fold_combine adds the partials to the profile in segment order.  A run cut
//          at a chunk end is cut at a micro-block boundary, so the sequence of adds does not depend on the chunk size: it
//          depends on the plan, on `first` and on the segment length, which follows from the device's compute units, nchan and
//          nbin (fold_moments_run) -- reproducible on one device and shape, not across them.
#include <string.h>

#include "engine_internal.h"
#include "fold_internal.h"
#include "fold_walk.h"

namespace dspsr_amd {

constexpr uint32_t MOM_NDIM = 14;             // floats per folded sample (FourthMoment.C:41)
constexpr uint32_t MOM_THREADS = 256;         // one workgroup: 4 waves, one per SIMD
// Bins per thread.  An owned bin costs 14 accumulators and 8 registers of plan cursor; with the chunk prefetch (32) and the 14
// values of the sample in flight, two bins stay near 100 VGPRs -- four workgroups per CU by registers and by LDS (4 x 36 KiB
// of 160) -- where four bins would take 60 more and halve that.  A row's bins beyond 512 go to further workgroups.
constexpr int MOM_BPT = 2;
constexpr uint32_t MOM_MB = 32;               // micro-block of the LONG association
constexpr uint32_t MOM_SEG_UNIT = 2048;       // LONG time segments are multiples of it
static_assert(MOM_MB == FOLD_MB && MOM_SEG_UNIT == FOLD_CHUNK, "the LONG association is fold.hip's (fold_walk.h fold_long_piece, fold_plan.h)");
constexpr uint32_t MOM_CHUNK_STOKES = 2048;   // samples per chunk image: 32 KiB of ndim 4 ...
constexpr uint32_t MOM_CHUNK_STREAM = 512;    // ... 28 KiB of ndim 14
constexpr uint32_t MOM_FM_SAMPLES = 256;      // k_fourth_moment: samples per workgroup

// one multiply rounded to nearest, kept apart from the add that follows it
static __device__ __forceinline__ float mul_rn(const float a, const float b)
{
#pragma clang fp contract(off)
  const float p = a * b;
  return p;
}

// the 14 floats of FourthMoment.C:62-75 from one Stokes sample
static __device__ __forceinline__ void moments_of(const float4 s, float (&v)[MOM_NDIM])
{
  v[0] = s.x; v[1] = s.y; v[2] = s.z; v[3] = s.w;
  v[4] = mul_rn(s.x, s.x); v[5] = mul_rn(s.x, s.y); v[6] = mul_rn(s.x, s.z); v[7] = mul_rn(s.x, s.w);
  v[8] = mul_rn(s.y, s.y); v[9] = mul_rn(s.y, s.z); v[10] = mul_rn(s.y, s.w);
  v[11] = mul_rn(s.z, s.z); v[12] = mul_rn(s.z, s.w);
  v[13] = mul_rn(s.w, s.w);
}

// component d of the 14 is in[MOM_I >> 2d & 3] (d < 4) or in[MOM_I ...] * in[MOM_J ...]: the loop order of FourthMoment.C:67-72
constexpr uint32_t mom_pack(const int which)
{
  uint32_t w = 0;
  int d = 4;
  for (int i = 0; i < 4; i++) w |= (uint32_t)i << (2 * i);
  for (int i = 0; i < 4; i++)
    for (int j = i; j < 4; j++, d++) w |= (uint32_t)(which ? j : i) << (2 * d);
  return w;
}
constexpr uint32_t MOM_I = mom_pack(0), MOM_J = mom_pack(1);

// dsp::FourthMoment::transformation.  Workgroup (x, chan) takes MOM_FM_SAMPLES samples: one 16-byte load per thread, the 14
// floats staged in LDS, the 56-byte samples written as coalesced 8-byte stores.  Rows: in 16-byte, out 8-byte aligned.
__global__ __launch_bounds__(MOM_FM_SAMPLES) void k_fourth_moment(const float* __restrict__ in, const uint64_t in_chan_stride,
                                                                   float* __restrict__ out, const uint64_t out_chan_stride,
                                                                   const uint64_t ndat)
{
  __shared__ __attribute__((aligned(16))) float stage[MOM_FM_SAMPLES * MOM_NDIM];
  const uint32_t tid = threadIdx.x;
  const uint64_t s0 = (uint64_t)blockIdx.x * MOM_FM_SAMPLES;
  const uint32_t n = (uint32_t)(ndat - s0 < MOM_FM_SAMPLES ? ndat - s0 : MOM_FM_SAMPLES);   // samples of this workgroup
  const float4* __restrict__ src = (const float4*)(in + blockIdx.y * in_chan_stride) + s0;
  float2* __restrict__ dst = (float2*)(out + blockIdx.y * out_chan_stride + s0 * MOM_NDIM);
  if (tid < n) {
    float v[MOM_NDIM];
    moments_of(src[tid], v);
#pragma unroll
    for (uint32_t d = 0; d < MOM_NDIM; d += 2) *(float2*)&stage[tid * MOM_NDIM + d] = make_float2(v[d], v[d + 1]);
  }
  __syncthreads();
  for (uint32_t q = tid; q < n * (MOM_NDIM / 2); q += MOM_FM_SAMPLES) dst[q] = ((const float2*)stage)[q];
}

// The moments fold.  grid (bin group, channel, LONG: time segment); thread t of bin group g owns bins g + ngroup * (t + j *
// MOM_THREADS), j < MOM_BPT, and walks each bin's time-ordered interval list with a cursor, as k_fold_chunked does.  The chunk
// image in LDS is what the loader read: CH samples of ndim 4 (STOKES) or ndim 14; LONG adds the (CH / MOM_MB) x 14 micro-block
// sums.  vec: the rows are 16-byte aligned (float4 loads); else the same image is filled float by float.
template <bool STOKES, bool LONG>
__global__ __launch_bounds__(MOM_THREADS) void k_fold_moments(const float* __restrict__ in, const uint64_t chan_stride, const uint32_t vec,
                                                               float* __restrict__ prof, const uint64_t prof_span, const uint32_t nbin,
                                                               const uint32_t* __restrict__ bin_start, const Interval* __restrict__ iv,
                                                               const uint64_t first, const uint64_t last /* [first,last): sample span of the plan */,
                                                               float* __restrict__ part /* LONG: [seg][chan][nbin][14] partial sums */,
                                                               const uint64_t seg_samples /* LONG: samples per blockIdx.z */)
{
  constexpr uint32_t IND = STOKES ? 4 : MOM_NDIM;                         // floats per sample of the input rows
  constexpr uint32_t CH = STOKES ? MOM_CHUNK_STOKES : MOM_CHUNK_STREAM;   // samples per chunk
  constexpr uint32_t NF4 = CH * IND / 4;                                  // float4 per chunk image
  constexpr uint32_t MAXR = NF4 / MOM_THREADS;                            // float4 per thread
  static_assert(MAXR * MOM_THREADS == NF4 && MOM_SEG_UNIT % CH == 0 && CH % MOM_MB == 0, "chunk image");
  constexpr uint32_t MS = (CH / MOM_MB) * MOM_NDIM;                       // micro-block sums (LONG)
  __shared__ __attribute__((aligned(16))) float img[CH * IND];
  __shared__ float mbs[LONG ? MS : 1];
  const uint32_t tid = threadIdx.x, bz = blockIdx.x, nz = gridDim.x, ichan = blockIdx.y;
  const float* __restrict__ row = in + ichan * chan_stride;
  float* __restrict__ out = LONG ? part + ((uint64_t)blockIdx.z * gridDim.y + ichan) * nbin * MOM_NDIM : prof + (uint64_t)ichan * prof_span;

  // the chunks of this workgroup: all of the span, or those of its time segment
  const uint32_t nchunk_all = (uint32_t)((last - first + CH - 1) / CH);
  const uint64_t seg0 = LONG ? (uint64_t)blockIdx.z * seg_samples : 0;                 // first sample of the segment, from `first`
  const uint32_t cbeg = LONG ? (uint32_t)(seg0 / CH) : 0u;
  const uint32_t nchunk = LONG ? ((seg0 + seg_samples) / CH < nchunk_all ? (uint32_t)((seg0 + seg_samples) / CH) : nchunk_all) : nchunk_all;

  uint32_t cur[MOM_BPT], end[MOM_BPT];
  Interval v0[MOM_BPT], v1[MOM_BPT];
  float acc[MOM_BPT][MOM_NDIM];
  bool touched[MOM_BPT];
  // (the cursor of fold_walk.h's FoldCursor, kept as its own code: with FoldCursor the stream loader, <false, false>, ran 24 % slower on the
  //  MI355X, everything else of the kernel unchanged -- profiles/HISTORY.md.)  "no interval" = offset ~0; always a global load with a
  //  clamped index
  auto load_iv = [&](const uint32_t i, const bool valid) -> Interval {
    Interval t = iv[valid ? i : 0u];
    if (!valid) { t.offset = ~0ull; t.hits = 0u; }
    return t;
  };
#pragma unroll
  for (int j = 0; j < MOM_BPT; j++) {
    const uint32_t b = bz + nz * (tid + j * MOM_THREADS);
    cur[j] = end[j] = 0;
    if (b < nbin) { cur[j] = bin_start[b]; end[j] = bin_start[b + 1]; }
    if constexpr (LONG) {
      // first interval of the bin that reaches into this segment (intervals are time ordered: binary search)
      uint32_t lo_i = cur[j], hi_i = end[j];
      while (lo_i < hi_i) {
        const uint32_t mid = (lo_i + hi_i) >> 1;
        const Interval t = iv[mid];
        if (t.offset + t.hits <= first + seg0) lo_i = mid + 1; else hi_i = mid;
      }
      cur[j] = lo_i;
    }
    touched[j] = LONG ? (b < nbin) : (cur[j] != end[j]);
    v0[j] = load_iv(cur[j], cur[j] < end[j]);
    v1[j] = load_iv(cur[j] + 1, cur[j] + 1 < end[j]);
#pragma unroll
    for (uint32_t d = 0; d < MOM_NDIM; d++) acc[j][d] = (!LONG && touched[j]) ? out[(uint64_t)b * MOM_NDIM + d] : 0.f;
  }

  // chunk c covers samples [first + c * CH, ...); first % 4 == 0 (host), so aligned rows give aligned chunks for either ndim
  const float* __restrict__ src0 = row + first * IND;
  const uint64_t nfl_total = (last - first) * IND;        // floats in the span: nothing behind them is read
  float4 pre[MAXR];
  auto fetch = [&](const uint32_t c) {
#pragma unroll
    for (uint32_t r = 0; r < MAXR; r++) {
      const uint64_t k = (uint64_t)c * NF4 + tid + r * MOM_THREADS, e = 4 * k;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (vec && e + 4 <= nfl_total) {
        v = ((const float4*)src0)[k];
      } else if (e < nfl_total) {                         // unaligned rows, or the ragged end of the span
        const uint64_t n = nfl_total - e;
        v.x = src0[e];
        if (n > 1) v.y = src0[e + 1];
        if (n > 2) v.z = src0[e + 2];
        if (n > 3) v.w = src0[e + 3];
      }
      pre[r] = v;
    }
  };
  // the 14 floats of sample h of the chunk image, added to one bin's accumulators: the ONE accumulation body of both loaders
  auto add_sample = [&](float (&a)[MOM_NDIM], const uint32_t h) {
    float v[MOM_NDIM];
    if constexpr (STOKES) {
      moments_of(((const float4*)img)[h], v);
    } else {
#pragma unroll
      for (uint32_t d = 0; d < MOM_NDIM; d += 2) {
        const float2 t = *(const float2*)&img[h * MOM_NDIM + d];
        v[d] = t.x; v[d + 1] = t.y;
      }
    }
#pragma unroll
    for (uint32_t d = 0; d < MOM_NDIM; d++) a[d] += v[d];
  };
  if (cbeg < nchunk) fetch(cbeg);
  for (uint32_t c = cbeg; c < nchunk; c++) {
    __syncthreads();                                      // previous chunk fully consumed
#pragma unroll
    for (uint32_t r = 0; r < MAXR; r++) ((float4*)img)[tid + r * MOM_THREADS] = pre[r];
    if (c + 1 < nchunk) fetch(c + 1);
    __syncthreads();
    if constexpr (LONG) {                                 // level 1: the sums of the aligned micro-blocks of this chunk, from zero
      for (uint32_t q = tid; q < MS; q += MOM_THREADS) {
        const uint32_t mb = q / MOM_NDIM, d = q - mb * MOM_NDIM;
        float sacc = 0.f;
        if constexpr (STOKES) {
          const uint32_t i = (MOM_I >> (2 * d)) & 3u, jj = (MOM_J >> (2 * d)) & 3u;
#pragma unroll 8
          for (uint32_t h = 0; h < MOM_MB; h++) {
            const float a = img[(mb * MOM_MB + h) * 4 + i], b = img[(mb * MOM_MB + h) * 4 + jj];
            sacc += d < 4 ? a : mul_rn(a, b);
          }
        } else {
#pragma unroll 8
          for (uint32_t h = 0; h < MOM_MB; h++) sacc += img[(mb * MOM_MB + h) * MOM_NDIM + d];
        }
        mbs[q] = sacc;
      }
      __syncthreads();
    }
    const uint64_t c0 = first + (uint64_t)c * CH, c1 = c0 + CH;
#pragma unroll
    for (int j = 0; j < MOM_BPT; j++) {
      while (v0[j].offset < c1) {                         // `none` has offset ~0 and ends the walk
        const Interval v = v0[j];
        const uint64_t lo = v.offset > c0 ? v.offset : c0;
        const uint64_t hi = v.offset + v.hits < c1 ? v.offset + v.hits : c1;
        const uint32_t s0 = (uint32_t)(lo - c0), s1 = s0 + (uint32_t)(hi - lo);       // samples [s0, s1) of the chunk
        if constexpr (LONG) {
          fold_long_piece(s0, s1, [&](const uint32_t h0, const uint32_t h1) { for (uint32_t h = h0; h < h1; h++) add_sample(acc[j], h); },
                          [&](const uint32_t m0, const uint32_t m1) {
                            for (uint32_t mb = m0; mb < m1; mb++)
#pragma unroll
                              for (uint32_t d = 0; d < MOM_NDIM; d++) acc[j][d] += mbs[mb * MOM_NDIM + d];
                          });
        } else {
#pragma unroll 2
          for (uint32_t h = s0; h < s1; h++) add_sample(acc[j], h);
        }
        if (v.offset + v.hits > c1) break;                // the interval continues in the next chunk (or segment)
        cur[j]++;
        v0[j] = v1[j];
        v1[j] = load_iv(cur[j] + 1, cur[j] + 1 < end[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MOM_BPT; j++) {
    const uint32_t b = bz + nz * (tid + j * MOM_THREADS);
    if (b < nbin && touched[j])
#pragma unroll
      for (uint32_t d = 0; d < MOM_NDIM; d++) out[(uint64_t)b * MOM_NDIM + d] = acc[j][d];
  }
}

}  // namespace dspsr_amd

using namespace dspsr_amd;

extern "C" int dspsr_amd_fourth_moment(dspsr_amd_ctx* ctx, const float* in_dev, uint64_t in_chan_stride, float* out_dev,
                                       uint64_t out_chan_stride, uint32_t nchan, uint64_t ndat)
{
  if (!ctx) return DSPSR_AMD_EINVAL;
  if (!in_dev || !out_dev) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fourth_moment: null buffer");
  if ((const void*)in_dev == (const void*)out_dev)      // Transformation <TimeSeries,TimeSeries> ("FourthMoment", outofplace), FourthMoment.C:25
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fourth_moment: out of place only (in == out)");
  if ((uintptr_t)in_dev % 16 || in_chan_stride % 4)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fourth_moment: input rows must be 16-byte aligned");
  if ((uintptr_t)out_dev % 8 || out_chan_stride % 2)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fourth_moment: output rows must be 8-byte aligned");
  if (in_chan_stride < ndat * 4 || out_chan_stride < ndat * MOM_NDIM)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fourth_moment: a channel stride is shorter than its row (ndat=%llu)",
                    (unsigned long long)ndat);
  if (nchan > 65535) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fourth_moment: nchan=%u > 65535", nchan);
  const uint64_t nblk = (ndat + MOM_FM_SAMPLES - 1) / MOM_FM_SAMPLES;
  if (nblk > 0x7fffffffull) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_fourth_moment: ndat=%llu too large", (unsigned long long)ndat);
  if (!nchan || !ndat) return DSPSR_AMD_OK;              // FourthMoment.C:49-50
  hipLaunchKernelGGL(k_fourth_moment, dim3((uint32_t)nblk, nchan), dim3(MOM_FM_SAMPLES), 0, ctx->stream, in_dev, in_chan_stride,
                     out_dev, out_chan_stride, ndat);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_fourth_moment: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

// Fold::Engine::fold of a 14-shape: the pending plan, bucketed by phase bin, walked by k_fold_moments.  stokes: in_dev holds
// ndim 4 Stokes rows (dspsr_amd_fold_fold_moments), else ndim 14 rows (dspsr_amd_fold_fold).  Same launch geometry either way.
int fold_moments_run(dspsr_amd_fold* f, const float* in_dev, uint64_t in_chan_stride, bool stokes, const char* who)
{
  dspsr_amd_ctx* ctx = f->ctx;
  if (!in_dev) return DSPSR_AMD_EINVAL;
  if (!f->profile) return ctx_fail(ctx, DSPSR_AMD_ESTATE, "%s: set_shape not called", who);
  if (f->ndim != MOM_NDIM || f->npol != 1)
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "%s: the profile is npol %u x ndim %u, not the npol 1 x ndim 14 of fourth moments", who,
                    f->npol, f->ndim);
  if (f->folding_nbin != f->nbin)    // Fold.C:806-809
    return ctx_fail(ctx, DSPSR_AMD_EINVAL, "dsp::Fold::fold folding_nbin != output->nbin (%u != %u)", f->folding_nbin, f->nbin);
  if (f->nchan > 65535) return ctx_fail(ctx, DSPSR_AMD_EINVAL, "%s: nchan=%u > 65535", who, f->nchan);
  if (f->binplan.empty()) return DSPSR_AMD_OK;             // send_binplan, FoldCUDA.cu:160-161
  PlanSlot* sl = nullptr;
  uint64_t first = 0, last = 0;
  uint32_t max_run = 0;
  int rc = fold_plan_to_device(f, who, &sl, &first, &last, &max_run);
  if (rc != DSPSR_AMD_OK) return rc;
  const uint32_t nbin = f->nbin, nchan = f->nchan;
  const uint32_t vec = ((uintptr_t)in_dev % 16 == 0 && in_chan_stride % 4 == 0) ? 1u : 0u;
  const FoldShape s = fold_moments_shape(nchan, nbin, first, last, max_run, ctx->ncu, MOM_NDIM, MOM_THREADS, MOM_BPT * MOM_THREADS);
  const bool lng = s.family == FOLD_MOMENTS_LONG;
  if (lng) {
    const size_t need = (size_t)s.nseg * nchan * nbin * MOM_NDIM;
    if (!grow_device_buffer(ctx->stream, f->part, f->part_floats, need))
      return ctx_fail(ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc of %zu partial-sum floats failed", who, need);
  }
  const dim3 grid(s.grid[0], s.grid[1], s.grid[2]);
#define MOM_LAUNCH(ST, LG) hipLaunchKernelGGL((k_fold_moments<ST, LG>), grid, dim3(s.threads), 0, ctx->stream, in_dev, in_chan_stride, vec, \
                                             f->profile, f->span, nbin, sl->d_bin_start, sl->d_iv, first, last, f->part, s.seg_len)
  if (stokes) { if (lng) MOM_LAUNCH(true, true); else MOM_LAUNCH(true, false); }
  else { if (lng) MOM_LAUNCH(false, true); else MOM_LAUNCH(false, false); }
#undef MOM_LAUNCH
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(ctx, DSPSR_AMD_EHIP, "%s: %s", who, hipGetErrorString(e));
  if (lng) {
    rc = fold_combine_partials(f, who, f->part, s.nseg, 0, nchan);
    if (rc != DSPSR_AMD_OK) return rc;
  }
  return fold_part_plan_submitted(f, sl);
}

extern "C" int dspsr_amd_fold_fold_moments(dspsr_amd_fold* f, const float* stokes_dev, uint64_t in_chan_stride)
{
  if (!f) return DSPSR_AMD_EINVAL;
  return fold_moments_run(f, stokes_dev, in_chan_stride, true, "dspsr_amd_fold_fold_moments");
}
