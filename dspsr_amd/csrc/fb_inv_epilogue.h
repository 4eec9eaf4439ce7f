// What the inverse passes k_inv_chan (fb_inv_chan.h) and k_rows_inv (fb_two_pass.hip) do behind their own loads and multiplies: the
// last stage's store with its three epilogues, and the fused fold -- the plan's way into LDS, the accumulator access, the pre-load of
// a thread's first accumulators and the fold phase.  What differs between the two kernels comes in as an argument (the channel of a
// staged row as a callable, logT3 as a value that is a constant in one of them); nothing here asks which kernel called it.
// Each kernel keeps its loads, its multiply, the place where the search carry is pre-loaded and every barrier.
#pragma once
#include "fb_common.h"
#include "fb_inv_walk.h"

namespace dspsr_amd {

// FOLD: the tile's detected samples are staged UNPADDED, channel after channel (16 bytes per sample), so that the
// samples of a phase bin's run are read at constant offsets from one base (the padded image cost four integer
// instructions per sample in a phase that only three of eight waves work in).  The channel stride is nkeep rounded up
// so that the T3 channels a quarter wave writes at once fall on different LDS banks.
// (many channels of a short transform: the rounded stride would not fit the exchange buffer -- 2*T3*nkeep words always do)
DEV uint32_t inv_fold_stride(const int logT3, const uint32_t nkeep, const uint32_t nthreads)
{
  const uint32_t fcr = (16u >> logT3) & 15u, fcs_r = ((nkeep + 15u - fcr) & ~15u) + fcr;
  return ((2u * fcs_r) << logT3) <= PTS * nthreads ? fcs_r : nkeep;
}

// The last stage's store (wgfft's `store` of one butterfly: column col = 2 * staged row + pol, elements p + k * pstride).  The output
// sample of element k is t0 + k * pstride, kept when 0 <= t < nkeep (negative t wraps).
//   FOLD    detected, staged with the stride fcs (inv_fold_stride) for inv_fold_phase
//   SEARCH  staged by ts_stage for ts_reduce.  One polarisation (!two): the pair's second half is not a signal -- for real input the
//           other output of the Hermitian split, zero but for rounding, 1e-7 of the spectrum's scale: its power moved the sum by an
//           ulp where a sample is small, tests/fuzz_search.py 300 702 case 68
//   neither complex or detected rows of channel out.chan0 + chan; the addresses are a base plus a multiple of a wave-uniform step, and
//           the output kind / layout is uniform: chosen once, outside the unrolled element loop (no branch per element)
// chan: the channel of the staged row, within this input channel's sub-band.  two: the second polarisation exists.
// TS_NPO (SEARCH): ts_stage's NPO -- 0 the square-law states, 4 the Coherence products.
template <bool FOLD, bool SEARCH, int TS_NPO = 0, class V>
DEV void inv_store(cf* lds, const FbGeom& g, const FbOut& out, const TsPart& tsp, const uint32_t fcs, const uint32_t chan,
                   const uint64_t part, const bool two, const uint32_t col, const uint32_t p, const uint32_t pstride, V& v)
{
  constexpr int R = sizeof(v) / sizeof(v[0]);
  const int32_t t0 = (int32_t)p - (int32_t)g.nfilt_pos;
  if constexpr (FOLD) {
    const uint32_t slo = col >> 1;
#pragma unroll
    for (int k = 0; k < R; k++) {
      const int32_t t = t0 + (int32_t)(k * pstride);
      if ((uint32_t)t >= g.nkeep) continue;
      float r[4];
      detect4(cx2_lo(v[k]), cx2_hi(v[k]), out.state, r);
      *(float4*)&lds[2 * (slo * fcs + (uint32_t)t)] = make_float4(r[0], r[1], r[2], r[3]);
    }
    return;
  }
  if constexpr (SEARCH) {
#pragma unroll
    for (int k = 0; k < R; k++) {
      const int32_t t = t0 + (int32_t)(k * pstride);
      if ((uint32_t)t >= g.nkeep) continue;
      ts_stage<TS_NPO>((float*)lds, out, tsp, col >> 1, (uint32_t)t, cx2_lo(v[k]), two ? cx2_hi(v[k]) : make_float2(0.f, 0.f));
    }
    return;
  }
  if (out.kind == FB_OUT_NONE) return;
  float* __restrict__ row = out.base + (out.chan0 + chan) * out.chan_stride;
  if (out.kind == FB_OUT_COMPLEX) {
    float2* __restrict__ o2 = (float2*)(row + part * out.part_step) + t0;
#pragma unroll
    for (int k = 0; k < R; k++) {
      if ((uint32_t)(t0 + (int32_t)(k * pstride)) >= g.nkeep) continue;
      fb_put_complex<true>(out, o2 + k * pstride, cx2_lo(v[k]), cx2_hi(v[k]), two);
    }
  } else if (out.ndim == 4) {
    const int64_t i0 = (int64_t)(part * g.nkeep) + t0;
#pragma unroll
    for (int k = 0; k < R; k++) {
      if ((uint32_t)(t0 + (int32_t)(k * pstride)) >= g.nkeep) continue;
      fb_put_detected_as<4, true>(out, row, i0 + k * pstride, cx2_lo(v[k]), cx2_hi(v[k]));
    }
  } else {
#pragma unroll
    for (int k = 0; k < R; k++) {
      const int32_t ts = t0 + (int32_t)(k * pstride);
      if ((uint32_t)ts >= g.nkeep) continue;
      fb_put_detected<true>(out, row, part * g.nkeep + (uint32_t)ts, cx2_lo(v[k]), cx2_hi(v[k]));
    }
  }
}

// ---- the fused fold ----------------------------------------------------------------------------------------------------------------
// Thread b of a workgroup owns work items w = b, b + blockDim, ...: (active phase bin w >> logT3, staged channel w % T3) of the part.
// It loads each touched accumulator from the device profile, adds the samples of the bin's intervals one by one in time order and
// stores it back.  A workgroup processes ALL parts of a tile (of its run of parts: fb_inv_walk.h) in order and launches are stream
// ordered, so every (chan, bin) sum has the association order of the CPU loop Fold.C:844-852, exactly as the stand-alone fold kernel
// (fold.hip) -- bit-identical results, without the 16 B/sample round trip of the detected time series through HBM.

// The plan's way into LDS.  Behind the twiddle tables (cf index plan_off, 16-byte aligned): two buffers of out.plan_cap plan entries
// {bin, first interval, count<<16 | hits0, offset0} (fold_internal.h), followed by a copy of the plan offsets of the parts THIS
// workgroup walks, psl[lp - p0] (FB_PSL_MAX words): a part's entries are then found without a dependent pair of global loads.
// (its run of a segmented launch: launches of up to 256 parts are cut into runs of at most FB_PSL_MAX - 1; the whole launch's offsets
//  did not fit, and every entry and accumulator of such launches -- the sub-band and -F 256:D geometries -- then came from global
//  memory in the fold phase)
struct InvPlan {
  uint32_t* psl;
  const uint4* fent_all;         // the plan's entries, behind its nparts_plan + 1 offsets
  uint4* buf;                    // the two LDS buffers
  bool use_psl, dma_ok;
  uint32_t fe0, fn;              // entries of the part about to be processed (inv_plan_fetch): first, count
};
// NS: stages of the transform.  The request for the next item's entries is issued from wgfft's `mid` hook behind the first exchange
// barrier, so it needs a second stage; single-stage transforms read their entries from global memory.
template <int NS>
DEV InvPlan inv_plan_begin(cf* lds, const uint32_t plan_off, const FbOut& out, const uint64_t part0, const InvWalk& w,
                           const uint32_t tid, const uint32_t nthreads)
{
  InvPlan pl;
  pl.buf = (uint4*)&lds[plan_off];
  pl.psl = (uint32_t*)&lds[plan_off + 4 * out.plan_cap];
  pl.fent_all = (const uint4*)(out.pstart + ((out.nparts_plan + 1 + 3) & ~3u));
  pl.use_psl = out.plan_cap > 0 && w.np + 1 <= FB_PSL_MAX;
  pl.dma_ok = NS >= 2 && pl.use_psl;
  pl.fe0 = pl.fn = 0;
  if (pl.use_psl) {
    for (uint32_t q = tid; q <= w.np; q += nthreads) pl.psl[q] = out.pstart[part0 + w.p0 + q];
    __syncthreads();
  }
  return pl;
}
// the entries of part lp, at the top of its tile: they travel with the chirp loads; the offsets come from the LDS copy
DEV void inv_plan_fetch(InvPlan& pl, const FbOut& out, const uint64_t part0, const InvWalk& w, const uint32_t lp)
{
  if (pl.use_psl) { pl.fe0 = pl.psl[lp - w.p0]; pl.fn = pl.psl[lp - w.p0 + 1] - pl.fe0; }
  else { pl.fe0 = out.pstart[part0 + lp]; pl.fn = out.pstart[part0 + lp + 1] - pl.fe0; }
}
// The active-bin entries of a part (16 bytes each, at most plan_cap <= blockDim of them) go from global memory STRAIGHT into
// their LDS buffer (global_load_lds_dwordx4: lane l of a wave lands at the wave's base + 16*l), asynchronously and
// without passing through registers.  Round 2 fetched them into a register at the top of the tile and stored them to
// LDS: the kernel sits at 256 registers, the value was spilled to scratch, and the ISA read `s_waitcnt vmcnt(0);
// global_load; s_waitcnt vmcnt(0); scratch_store; ...; scratch_load; s_waitcnt vmcnt(0); ds_write` -- two exposed memory
// round trips on the two waves everyone then waits for at the first barrier.  The entries of the NEXT item are now
// requested in the middle of the current tile's transform (behind a barrier that the previous readers of that buffer
// have passed; double buffered: slower waves may still be folding the previous tile from the other half) and are waited for,
// together with the prefetched tile, at the top of the next one.
DEV void inv_plan_dma(const InvPlan& pl, const FbOut& out, const InvWalk& w, const uint32_t lp, const uint32_t buf, const uint32_t tid)
{
  const uint32_t fe0 = pl.psl[lp - w.p0], fn = pl.psl[lp - w.p0 + 1] - fe0;
  if (fn <= out.plan_cap && tid < fn)
    lds_dma_b128((const void*)(pl.fent_all + fe0 + tid), lds_byte_addr(pl.buf + buf * out.plan_cap + (tid & ~63u)));
}

// The part of the tile being folded: its nact active bins' entries, in LDS buffer jt & 1 when they fit (in_lds), else at `ent`.
struct InvFoldPart {
  uint32_t nact;
  const uint4* ent;
  const uint4* planl;
  bool in_lds;
};
DEV InvFoldPart inv_fold_part(const InvPlan& pl, const FbOut& out, const uint32_t jt)
{
  InvFoldPart fp;
  fp.nact = pl.fn;
  fp.ent = pl.fent_all + pl.fe0;
  fp.planl = pl.buf + (jt & 1) * out.plan_cap;
  fp.in_lds = pl.dma_ok && pl.fn <= out.plan_cap;
  return fp;
}

// accumulator of (channel cl, phase bin b): one float4, or -- profile of npol 2 x ndim 2 -- a float2 in each of the channel's two
// rows; run 0 of the launch (seg == 0) folds onto the profile, the others onto the partial profiles of a segmented launch, packed in
// the same shape (rows of nbin bins).  cl: channel within this input channel's sub-band.
struct InvAcc {
  bool planes2;                  // uniform
  uint64_t plane;                // floats between the two rows of a channel
};
DEV InvAcc inv_acc(const FbOut& out, const uint32_t seg) { return {out.prof_planes == 2, seg == 0 ? out.plane_stride : 2ull * out.nbin}; }
DEV float* inv_acc_row(const FbGeom& g, const FbOut& out, const uint32_t seg, const uint32_t cl)
{
  return (float*)(seg == 0 ? (float4*)out.base + (uint64_t)(out.chan0 + cl) * out.prof_span4
                           : (float4*)out.part + ((uint64_t)(seg - 1) * g.C + cl) * out.nbin);
}
DEV float4 inv_acc_load(const InvAcc& ac, float* row, const uint32_t b)
{
  if (ac.planes2) {
    const float2 u = *(const float2*)(row + 2 * b), v = *(const float2*)(row + ac.plane + 2 * b);
    return make_float4(u.x, u.y, v.x, v.y);
  }
  return *(const float4*)(row + 4 * b);
}
DEV void inv_acc_store(const InvAcc& ac, float* row, const uint32_t b, const float4 a)
{
  if (ac.planes2) {
    *(float2*)(row + 2 * b) = make_float2(a.x, a.y);
    *(float2*)(row + ac.plane + 2 * b) = make_float2(a.z, a.w);
  } else {
    *(float4*)(row + 4 * b) = a;
  }
}

// The accumulators of a thread's first NPRE work items (one is nearly always its only one; two where a part's active bins x
// channels exceed the workgroup, k_rows_inv with >= 8 channels per tile) are requested in the middle of the transform -- behind two
// barriers, so the previous part's stores of this workgroup are visible -- and arrive while the last stage runs, instead of costing
// a memory round trip in the fold phase.
// Only when the part's plan entries are in LDS: the accumulator's address then depends on an LDS read alone.  With the entry
// possibly coming from global memory (a select, or two branches that the compiler merges again) the load sat behind
// s_waitcnt vmcnt(0) -- a wait for the whole prefetch of the next tile, in the middle of the transform, on exactly the three waves
// that also fold.
// chan_of(slo): channel of staged row slo.  wstep: the workgroup's threads.
template <int NPRE, class ChanOf>
DEV void inv_acc_preload(const FbGeom& g, const FbOut& out, const InvAcc& ac, const uint32_t seg, const InvFoldPart& fp, const int logT3,
                         const uint32_t tid, const uint32_t wstep, uint4 (&en_pre)[NPRE], float4 (&acc_pre)[NPRE], ChanOf&& chan_of)
{
#pragma unroll
  for (int k = 0; k < NPRE; k++) {
    const uint32_t w = tid + k * wstep;
    if (fp.in_lds && w < (fp.nact << logT3)) {
      en_pre[k] = fp.planl[w >> logT3];
      acc_pre[k] = inv_acc_load(ac, inv_acc_row(g, out, seg, chan_of(w & ((1u << logT3) - 1))), en_pre[k].x);
    }
  }
}

// The fold phase, behind the barrier that ends the staging of the tile's detected samples (the barrier in front of the next tile's
// first exchange write ends this read phase).  The samples of an interval are fetched from LDS eight at a time (independent loads)
// and then added one after the other, so the sum keeps the time order; further intervals of the bin in this part (rare) come from
// out.piv.  pre: en_pre / acc_pre hold the thread's first NPRE work items (inv_acc_preload).
template <int NPRE, class ChanOf>
DEV void inv_fold_phase(const cf* lds, const FbGeom& g, const FbOut& out, const InvAcc& ac, const uint32_t seg, const InvFoldPart& fp,
                        const bool pre, const int logT3, const uint32_t fcs, const uint32_t tid, const uint32_t wstep,
                        const uint4 (&en_pre)[NPRE], const float4 (&acc_pre)[NPRE], ChanOf&& chan_of)
{
  static_assert(NPRE == 1 || NPRE == 2, "inv_fold_phase: one or two pre-loaded accumulators");
  // (the pre-loaded values are read here, once, as values: read from the arrays inside the branches below, the compiler merged the
  //  read of acc_pre[0] with the profile load of the other branch into one load through a pointer that is either -- and the array
  //  stayed in scratch, 16 bytes in every fused kernel that pre-loads one accumulator)
  const uint4 en0 = en_pre[0], en1 = en_pre[NPRE - 1];
  const float4 acc0 = acc_pre[0], acc1 = acc_pre[NPRE - 1];
  for (uint32_t w = tid; w < (fp.nact << logT3); w += wstep) {
    const uint32_t slo = w & ((1u << logT3) - 1);
    uint4 en;
    float4 acc;
    if (pre && w == tid) {
      en = en0;
      acc = acc0;
    } else if (NPRE == 2 && pre && w == tid + wstep) {
      en = en1;
      acc = acc1;
    } else {
      en = fp.in_lds ? fp.planl[w >> logT3] : fp.ent[w >> logT3];
      acc = inv_acc_load(ac, inv_acc_row(g, out, seg, chan_of(slo)), en.x);
    }
    const uint32_t nint = en.z >> 16;
    float* __restrict__ pp = inv_acc_row(g, out, seg, chan_of(slo));
    uint32_t off = en.w, hits = en.z & 0xffffu;
    for (uint32_t i = 0;;) {
      const float4* __restrict__ src = (const float4*)&lds[2 * (slo * fcs + off)];     // consecutive samples: constant offsets
      uint32_t h = 0;
      for (; h + 8 <= hits; h += 8) {
        float4 sm[8];
#pragma unroll
        for (int q = 0; q < 8; q++) sm[q] = src[h + q];
#pragma unroll
        for (int q = 0; q < 8; q++) { acc.x += sm[q].x; acc.y += sm[q].y; acc.z += sm[q].z; acc.w += sm[q].w; }
      }
      for (; h < hits; h++) {
        const float4 sm = src[h];
        acc.x += sm.x; acc.y += sm.y; acc.z += sm.z; acc.w += sm.w;
      }
      if (++i >= nint) break;
      const Interval iv = out.piv[en.y + i];
      off = (uint32_t)iv.offset; hits = iv.hits;
    }
    inv_acc_store(ac, pp, en.x, acc);
  }
}

// ---- the fused square-law fold (EPI == 3: Intensity, PPQQ; dspsr -d 1, -d 2) -------------------------------------------------------
// The same plan, the same item walk, the same time order; what differs is the sample.  A kept sample is detected with sqld() and
// staged as NPO = out.prof_planes floats: PP + QQ (Detection.C:285-300; the power of its one polarisation where the object has one:
// the pair's second half is no signal, see SEARCH above), or (PP, QQ).  Staged UNPADDED, channel after channel, as the 16-byte
// samples are: fcs samples from one channel to the next.  A group of lanes stores 128 bytes at once (32 lanes of ds_write_b32, 16
// of ds_write_b64): the T3 channels x S / T3 consecutive samples of such a group, S = 32 / NPO samples, fall on different banks
// when the channel stride is S / T3 samples more than a multiple of S.
// The accumulators are single floats: row (channel c, q) of the profile starts at out.base + (c * NPO + q) * out.chan_stride (the
// fold's row span in floats, in the field the fold form did not use), a run's partial profile is packed [chan][NPO][nbin].  ANY
// float-aligned profile fuses: there is no condition on the base address, the span or the padding of a bound profile.
DEV uint32_t inv_foldq_stride(const int logT3, const uint32_t nkeep, const uint32_t nthreads, const uint32_t npo)
{
  const uint32_t S = 32u / npo, fcr = (S >> logT3) & (S - 1u), fcs_r = ((nkeep + S - 1u - fcr) & ~(S - 1u)) + fcr;
  return ((npo * fcs_r) << logT3) <= 2u * PTS * nthreads ? fcs_r : nkeep;      // (npo * T3 * nkeep words always fit: 4 * T3 * M do)
}

template <class V>
DEV void inv_store_sq(cf* lds, const FbGeom& g, const FbOut& out, const uint32_t fcs, const bool two, const uint32_t col, const uint32_t p,
                      const uint32_t pstride, V& v)
{
  constexpr int R = sizeof(v) / sizeof(v[0]);
  const int32_t t0 = (int32_t)p - (int32_t)g.nfilt_pos;
  float* __restrict__ row = (float*)lds + (size_t)(col >> 1) * fcs * out.prof_planes;
  if (out.prof_planes == 2) {                 // uniform: chosen outside the unrolled element loop
#pragma unroll
    for (int k = 0; k < R; k++) {
      const int32_t t = t0 + (int32_t)(k * pstride);
      if ((uint32_t)t >= g.nkeep) continue;
      *(float2*)&row[2 * (uint32_t)t] = make_float2(sqld(cx2_lo(v[k])), sqld(cx2_hi(v[k])));
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < R; k++) {
    const int32_t t = t0 + (int32_t)(k * pstride);
    if ((uint32_t)t >= g.nkeep) continue;
    const float pp = sqld(cx2_lo(v[k]));
    row[(uint32_t)t] = two ? __fadd_rn(pp, sqld(cx2_hi(v[k]))) : pp;
  }
}

// row q = 0 of channel cl (within this input channel's sub-band), and the floats from it to row q = 1
DEV float* inv_accq_row(const FbGeom& g, const FbOut& out, const uint32_t seg, const uint32_t cl)
{
  return seg == 0 ? out.base + (uint64_t)(out.chan0 + cl) * out.prof_planes * out.chan_stride
                  : out.part + ((uint64_t)(seg - 1) * g.C + cl) * out.prof_planes * out.nbin;
}

// The fold phase of inv_fold_phase on NPO floats per sample: a work item is (active bin, staged channel) and carries the NPO
// accumulators of the channel's rows, so the plan is walked once for PP and QQ and a sample is one LDS read (ds_read_b64).  No
// accumulator is pre-loaded in the middle of the transform (inv_acc_preload): the item loads its own, at the cost of one
// memory round trip per part in the waves that fold.
template <int NPO, class ChanOf>
DEV void inv_foldq_phase(const cf* lds, const FbGeom& g, const FbOut& out, const uint32_t seg, const InvFoldPart& fp, const int logT3,
                         const uint32_t fcs, const uint32_t tid, const uint32_t wstep, ChanOf&& chan_of)
{
  static_assert(NPO == 1 || NPO == 2, "inv_foldq_phase: one or two floats per sample");
  const float* __restrict__ stg = (const float*)lds;
  const uint64_t rs = seg == 0 ? out.chan_stride : out.nbin;           // floats from row q to row q + 1
  for (uint32_t w = tid; w < (fp.nact << logT3); w += wstep) {
    const uint32_t slo = w & ((1u << logT3) - 1);
    const uint4 en = fp.in_lds ? fp.planl[w >> logT3] : fp.ent[w >> logT3];
    float* __restrict__ pp = inv_accq_row(g, out, seg, chan_of(slo)) + en.x;
    float acc[NPO];
#pragma unroll
    for (int q = 0; q < NPO; q++) acc[q] = pp[q * rs];
    const uint32_t nint = en.z >> 16;
    uint32_t off = en.w, hits = en.z & 0xffffu;
    for (uint32_t i = 0;;) {
      const float* __restrict__ src = stg + (size_t)(slo * fcs + off) * NPO;            // consecutive samples: constant offsets
      uint32_t h = 0;
      for (; h + 8 <= hits; h += 8) {
        float sm[8][NPO];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          if constexpr (NPO == 2) { const float2 s2 = *(const float2*)&src[2 * (h + q)]; sm[q][0] = s2.x; sm[q][1] = s2.y; }
          else sm[q][0] = src[h + q];
        }
#pragma unroll
        for (int q = 0; q < 8; q++)
#pragma unroll
          for (int d = 0; d < NPO; d++) acc[d] += sm[q][d];
      }
      for (; h < hits; h++) {
        if constexpr (NPO == 2) { const float2 s2 = *(const float2*)&src[2 * h]; acc[0] += s2.x; acc[1] += s2.y; }
        else acc[0] += src[h];
      }
      if (++i >= nint) break;
      const Interval iv = out.piv[en.y + i];
      off = (uint32_t)iv.offset; hits = iv.hits;
    }
#pragma unroll
    for (int q = 0; q < NPO; q++) pp[q * rs] = acc[q];
  }
}

}  // namespace dspsr_amd
