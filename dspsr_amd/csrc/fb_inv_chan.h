// Convolving filterbank, inverse pass of the three-pass path (k_inv_chan); instantiated by fb_inv_chan.hip (plain output)
// and fb_inv_chan_fold.hip (fused fold): two translation units so that the two families compile in parallel.
#pragma once
#include "fb_inv_epilogue.h"

namespace dspsr_amd {

// ------------------------------------------------------------------------------------ P3

// T3 output channels (both polarisations) of one part: the two polarisations of every (channel, bin) x chirp, inverse M-point
// FFT, keep window, complex output or fused detection.  Columns are (channel, pol) pairs: col = 2*slo + pol, so
// the two butterflies a thread owns are the two polarisations of the same (channel, bin):
// one load (and one chirp factor) serves both and detection needs no cross-lane traffic.
// Where the two polarisations come from:
//   PRESPLIT (real dual-polarisation input, the default where the host's condition holds -- filterbank.hip fb_takes_presplit):
//     pass 2 has already formed the Hermitian split and left X'[c/T3][p(m)][c%T3][pol] (fb_row_map.h).  One ascending 16-byte load
//     per element; x = (pol0, pol1) * chirp.  No mirror stream, no lane exchange, no split arithmetic in this pass.
//   otherwise: from X.  Real input: Hermitian split of spectrum rows s and Rr-1-s, a second, descending load stream (a, b) --
//     in aligned 16-byte pairs exchanged between lane pairs where a tile is two channels (PAIR16); complex input: the rows of
//     the two sequences.  This is the form of complex input, odd-factor lengths and of split_in_inverse = 1.
// Items (fb_inv_walk.h): part fastest, so one XCD re-reads a tile's chirp rows from its L2 for every part; FOLD and search mode walk
// the parts of a tile in order.
// FOLD: the detected samples of the tile (T3 channels x nkeep samples, one float4 each) are staged in the
// exchange buffer instead of being written out, and folded at once (fb_inv_epilogue.h).
// EPI: 0 = complex or detected output written by the last stage; 1 (FOLD) = fused fold; 2 = search mode (FB_OUT_SEARCH): square-law
// detection + time scrunch of the detected stream (digifil -F N:D, LoadToFil.C:185-222,250-304), staged like the fold's samples and
// reduced by ts_reduce (fb_common.h).  Both walk the parts of a tile in order (the fold's profile, the scrunch's carry).
// 3 = fused fold of the square-law states (Intensity, PPQQ: dspsr -d 1, -d 2; fb_inv_chan_fold_sq.hip): FOLD's walk and plan, the
// samples staged as one or two floats and added to scalar accumulators (fb_inv_epilogue.h, "the fused square-law fold").
// EPIP = EPI + 4 * PRESPLIT: the pre-split forms are k_inv_chan<., 4 | 5 | 6 | 7, .>, the others keep the names they had.  (As a
// fourth template parameter the flag renames every instantiation; as a device body behind two kernels the fused pre-split form
// came out with 12 bytes of scratch: profiles/r07_experiments.txt.)
// EPIP bit 8 (FB_EPI_MATRIX, plain output only: k_inv_chan<., 8 | 12, .>, fb_inv_chan_matrix.hip): the response is one Jones matrix
// per bin (Response::operate(data1, data2), Response.C:515-585) -- `kernel` then points at 32 bytes per bin, [channel][bin], as two
// 16-byte halves (f11, f21) and (f22, f12): the host's array as it stands (Response.C:614-640).  A tile's matrices would be 128
// registers per thread, so they are not kept: every item streams them in groups of FB_MATRIX_GROUP elements, one group ahead of
// the group being multiplied, and a workgroup always walks the parts of a tile one after the other so that the re-reads find the
// tile's rows warm.
constexpr int FB_EPI_PRESPLIT = 4;
constexpr int FB_EPI_MATRIX = 8;
// EPIP bit 16 (FB_EPI_COHERENCE, search mode only: k_inv_chan<., 18 | 22, .>, fb_inv_chan_search_coh.hip): the search epilogue on the
// four Coherence products PP, QQ, Re PQ*, Im PQ* (digifits -p 4, digifil -d 4) -- four staged rows and four carries per channel,
// detection and row count compile-time (ts_stage<4>, ts_reduce<4>).  The square-law forms <., 2 | 6, .> do not see the bit: every
// use of it below is `if constexpr` or a constant that is theirs when it is clear.
constexpr int FB_EPI_COHERENCE = 16;
constexpr int FB_MATRIX_GROUP = 4;     // elements per response load group: 32 registers, two groups live at a time

// (d1', d2') = J (d1, d2) for the two polarisations a cx2 holds, h0 = (f11, f21), h1 = (f22, f12).  Each output is the scalar
// path's complex multiply of its own polarisation with the diagonal element (cmul on a cx2 rounds like cmuls), then the two
// real products of the other polarisation's term added one after the other as Response.C:570-582 writes them -- with
// f12 = f21 = 0 every one of those adds 0 * d through an fma, so diag(k, k) gives the bits of the scalar response k.
// (The reference forms d2' as f21 d1 + f22 d2; here the sum starts from f22 d2 for that equality to hold on both outputs.)
DEV cx2 cmatmul(const cx2 d, const float4 h0, const float4 h1)
{
  const cx2 dg = make_cx2(make_float2(h0.x, h0.y), make_float2(h1.x, h1.y));    // (f11, f22)
  const cx2 of = make_cx2(make_float2(h1.z, h1.w), make_float2(h0.z, h0.w));    // (f12, f21)
  cx2 sw;                                                                        // (d2, d1)
  sw.x = (v2f){d.x[1], d.x[0]};
  sw.y = (v2f){d.y[1], d.y[0]};
  cx2 r = cmul(d, dg);
  r.x = r.x + of.x * sw.x;
  r.x = r.x - of.y * sw.y;
  r.y = r.y + of.y * sw.x;
  r.y = r.y + of.x * sw.y;
  return r;
}

template <int LOGF, int EPIP, int LOGT>
__global__ __launch_bounds__(512) void k_inv_chan(const FbGeom g, const cf* __restrict__ X,
                                                  const cf* __restrict__ kernel, const FbOut out,
                                                  const cf* __restrict__ tw, const uint64_t part0,
                                                  const uint32_t nparts, const uint32_t run)
{
  constexpr int EPI = EPIP & 3;
  constexpr bool PRESPLIT = (EPIP & FB_EPI_PRESPLIT) != 0;
  constexpr bool MATRIX = (EPIP & FB_EPI_MATRIX) != 0;
  static_assert(!MATRIX || EPI == 0, "the matrix response has the plain epilogue only");
  constexpr bool COH = (EPIP & FB_EPI_COHERENCE) != 0;
  static_assert(!COH || EPI == 2, "the Coherence products are a form of the search epilogue");
  constexpr int TS_NPO = COH ? 4 : 0;       // ts_stage / ts_reduce: 0 = npol_out from out.state (Intensity, PPQQ)
  typedef FftPlan<LOGF> P;
  constexpr bool FOLD = EPI == 1, SEARCH = EPI == 2;
  constexpr bool FOLDQ = EPI == 3;          // the fused square-law fold: walks and plans as FOLD, stages and adds floats
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  uint32_t tid = threadIdx.x;
  const int logT3 = LOGT >= 1 ? LOGT - 1 : g.logT3;
  const int logT = logT3 + 1;
  const uint32_t T = 1u << logT, T3 = 1u << logT3, M = 1u << LOGF, Rr = g.nsub << g.logR;     // (nsub = 3, 5: not a power of two)
  const uint64_t L = (uint64_t)M * Rr;
  const uint32_t nseq = g.real_input ? 1 : g.npol;
  const int logX3 = g.logX3;                    // X layout: element (row, m) at ((row >> logX3)*M + m) << logX3 | row % X3
  const uint32_t X3 = 1u << logX3;
  const uint32_t ntile = g.C >> logT3;
  auto xi = [&](const uint32_t row, const uint32_t m) -> uint64_t {
    return ((((uint64_t)(row >> logX3) << LOGF) + m) << logX3) | (row & (X3 - 1));
  };
  struct Abk { cf a, b; };   // the chirp is fetched at the start of the item (keeps the prefetch at 64 registers); PRESPLIT: (pol0, pol1)

  // chunk < 0: all elements; otherwise the elements i with i % NCHUNK == chunk (the prefetch of the next tile is
  // issued in NCHUNK groups spread over the transform, see wgfft_stage)
  constexpr int NCHUNK = P::NS + 1;
  // T = 4 columns = 2 channels x 2 polarisations per tile: the two channels' elements are loaded as aligned 16-byte pairs and
  // the halves exchanged between the lane pair.  -3.7 % where the detected or complex output is written; in the fused
  // kernel it cost 1.6 % while the chirp was still loaded per part (round 1) and gains 5.7 % now that it stays in registers
  // (profiles/r02_experiments.txt, item 23)
  constexpr bool PAIR16 = !PRESPLIT && LOGT == 2 && P::G1 == 2;
  const bool pair16 = PAIR16 && g.real_input && logX3 == 1;
  cf special = make_float2(0.f, 0.f);                   // mirror element of bin 0 (pair16 path)
  typedef InvItem Item;                                  // (tile of channels, part of the launch): fb_inv_walk.h
  auto fetch = [&](const Item item, Abk (&raw)[PTS / 2], const int chunk) {
    const uint32_t tile = item.tile;
    const cf* __restrict__ X0s = X + (uint64_t)item.lp * nseq * L;
    // element i of a thread's first-stage butterfly is bin m = mb + i*MS of one (channel, pol pair) column, so
    // every address is a base plus a multiple of a wave-uniform step: no per-element index arithmetic, no
    // divergent code between the loads (the m = 0 mirror element, the only irregular one, can only be i = 0)
    constexpr uint32_t MS = 1u << (LOGF - P::LOGR1);
    const int64_t step = (int64_t)MS << logX3;
    if constexpr (PRESPLIT) {
      // X' holds (pol0, pol1) of (channel s, bin m) as the 16-byte element xi(s, rm_xrow(m)): L/2 of them per part.  The bins
      // m = mb + i*MS of a thread are below M/2 for i < R1/2 and above it -- one place down -- for the others; bin M/2 itself
      // (mb = 0, i = R1/2), the only irregular one, has the last place
      // (a uniform base and 32-bit element offsets within the part -- L / 2 <= 2^25 elements: two address registers per pair
      //  of columns; as three pointers the fused form spilled 12 bytes)
      const float4* __restrict__ X4 = (const float4*)X + (uint64_t)item.lp * (L >> 1);
      const uint32_t step4 = MS << logX3;
#pragma unroll
      for (int g2 = 0; g2 < P::G1; g2 += 2) {
        const uint32_t eb = P::G1 * tid + g2, s = tile * T3 + ((eb & (T - 1)) >> 1), mb = eb >> logT;
        const uint32_t o0 = (uint32_t)xi(s, mb);
        const uint32_t omid = mb ? o0 + (P::R1 / 2) * step4 - X3 : (uint32_t)xi(s, M - 1);
#pragma unroll
        for (int i = 0; i < P::R1; i++) {
          if (chunk >= 0 && i % NCHUNK != chunk) continue;
          const float4 v = ld_stream(i < P::R1 / 2 ? X4 + i * step4 + o0 : i == P::R1 / 2 ? X4 + omid : (X4 + (i * step4 - X3)) + o0);
          Abk r;
          r.a = make_float2(v.x, v.y);
          r.b = make_float2(v.z, v.w);
          raw[(g2 / 2) * P::R1 + i] = r;
        }
      }
      return;
    }
    if constexpr (PAIR16) {
      if (pair16) {
        // Two channels per tile and X3 = 2: the elements of lanes 2j (channel 0) and 2j+1 (channel 1) for the same bin
        // are one aligned 16-byte pair, in both streams.  Lane parity q loads the pairs of the elements i = 2u + q --
        // 16 B per lane, half the load instructions (8-byte-per-lane streams run at 5.6 TB/s, 16-byte ones at 7.1 on this
        // chip, tools/load_width_probe.hip); the halves are exchanged between the two lanes when the tile is consumed.
        const uint32_t q = tid & 1, mb = tid >> 1;
        const uint32_t m0 = mb + q * MS;                                  // bin of element i = q
        const cf* __restrict__ pa2 = X0s + ((((uint64_t)tile << LOGF) + m0) << 1);
        const uint64_t rowb = (uint64_t)((Rr >> 1) - 1 - tile) << LOGF;   // row pair of the mirror rows Rr-1-s
        const cf* __restrict__ pb2 = X0s + ((rowb + (M - m0)) << 1);        // mirror bin M - m of element i = q
#pragma unroll
        for (int u = 0; u < P::R1 / 2; u++) {
          const float4 A = ld_stream((const float4*)(pa2 + (int64_t)u * 4 * MS));
          // bin 0 has its own mirror (loaded below): its pair would lie past the row, read the one before instead
          const float4 B = ld_stream((const float4*)((u == 0 && m0 == 0 ? pb2 - 2 : pb2) - (int64_t)u * 4 * MS));
          raw[2 * u].a = make_float2(A.x, A.y); raw[2 * u + 1].a = make_float2(A.z, A.w);
          raw[2 * u].b = make_float2(B.x, B.y); raw[2 * u + 1].b = make_float2(B.z, B.w);
        }
        const uint32_t s = tile * T3 + q;
        special = ld_stream(mb == 0 ? X0s + xi(s ? Rr - s : 0u, 0) : X0s + xi(Rr - 1 - s, M - mb));
        return;
      }
    }
#pragma unroll
    for (int g2 = 0; g2 < P::G1; g2 += 2) {
      const uint32_t eb = P::G1 * tid + g2;
      const uint32_t slo = (eb & (T - 1)) >> 1, mb = eb >> logT;
      const uint32_t s = tile * T3 + slo;
      const cf* __restrict__ pa = X0s + xi(s, mb);
      const cf* __restrict__ pb = g.real_input ? X0s + xi(Rr - 1 - s, M - mb) : pa + (g.npol == 2 ? L : 0);
      const int64_t stepb = g.real_input ? -step : step;
      const cf* __restrict__ pb0 = (g.real_input && mb == 0) ? X0s + xi(s ? Rr - s : 0u, 0) : pb;
#pragma unroll
      for (int i = 0; i < P::R1; i++) {
        if (chunk >= 0 && i % NCHUNK != chunk) continue;
        Abk r;
        r.a = ld_stream(pa + i * step);
        r.b = ld_stream(i == 0 ? pb0 : pb + i * stepb);
        raw[(g2 / 2) * P::R1 + i] = r;
      }
    }
  };
  // chirp of a tile (fetched at the start of the item: keeps the prefetch at 64 registers)
  auto load_chirp = [&](const Item item, cf (&kk)[MATRIX ? 1 : PTS / 2]) {
    if constexpr (MATRIX) return;
    const uint32_t ktile = item.tile;
    if (kernel) {                                 // uniform; outside the unrolled loads (no per-load branch / vmcnt(0))
      constexpr uint32_t MS = 1u << (LOGF - P::LOGR1);
#pragma unroll
      for (int g2 = 0; g2 < P::G1; g2 += 2) {
        const uint32_t eb = P::G1 * tid + g2;
        const cf* __restrict__ pk = kernel + ((uint64_t)(ktile * T3 + ((eb & (T - 1)) >> 1)) << LOGF) + (eb >> logT);
#pragma unroll
        for (int i = 0; i < P::R1; i++) kk[(g2 / 2) * P::R1 + i] = pk[i * MS];
      }
    } else {
#pragma unroll
      for (int i = 0; i < PTS / 2; i++) kk[i] = make_float2(1.f, 0.f);
    }
  };

  const uint32_t ltw_off = lds_pad(PTS * blockDim.x) + 8;      // behind the exchange buffer (16-byte aligned)
  ltw_fill<LOGF>(lds, ltw_off, tw, tid, blockDim.x);
  const uint32_t plan_off = (ltw_off + ltw_entries_dev<LOGF>() + 1) & ~1u;    // FOLD: the plan's LDS, behind the twiddle tables
  uint32_t jt = 0;                                              // tiles done by this workgroup
  Item item, next;
  uint32_t j = 0;
  // (MATRIX and the XCD remap of the fused fold's tiles are this kernel's own parameters of the walk)
  const InvWalk walk = inv_walk(EPI != 0, MATRIX, FOLD || FOLDQ ? out.nseg : 1u, nparts, ntile, run, gridDim.x, blockIdx.x, FOLD || FOLDQ ? logX3 - logT3 : 0);
  const uint32_t fseg = walk.seg;
  auto next_item = [&](const uint32_t jj, Item& it) -> bool { return inv_walk_item(walk, jj, it); };
  [[maybe_unused]] InvPlan plan = {};
  if constexpr (FOLD || FOLDQ) {
    if (walk.np == 0) return;
    plan = inv_plan_begin<P::NS>(lds, plan_off, out, part0, walk, tid, blockDim.x);
  }
  if (!next_item(j, item)) return;
  Abk raw[PTS / 2];
  fetch(item, raw, -1);
  cf kk[MATRIX ? 1 : PTS / 2];          // chirp of the current tile (MATRIX: none, the response is streamed per item)
  uint32_t kk_tile = ~0u;
  if constexpr (FOLD || FOLDQ) {
    if (plan.dma_ok) inv_plan_dma(plan, out, walk, item.lp, 0, tid);
  }

  FB_ST_BEGIN(3);
  for (;;) {
    asm volatile("" : "+v"(tid));   // per-tile index math stays inside the loop (see wgfft)
    cx2 x[NPAIR];
    FB_ST(3, 0);                     // (waits for the prefetched tile first)
    {
      // FOLD: a workgroup walks the parts of ITS tile, so consecutive items share the chirp rows: they are loaded when
      // the tile changes and stay in registers (the load and its latency were 22 % of the tile, profiles/r02c_*)
      if constexpr (!MATRIX) {
        if (item.tile != kk_tile) {
          load_chirp(item, kk);
          kk_tile = item.tile;
        }
      }
      if constexpr (FOLD || FOLDQ) {
        inv_plan_fetch(plan, out, part0, walk, item.lp);
        // the entries requested during the previous tile (or in front of the loop) have landed once every older load has
        // -- they were issued half a tile ago, behind the prefetch of this tile
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if constexpr (PAIR16) {
        if (pair16) {                       // hand the other channel's halves of the 16-byte pairs to the neighbour lane
          const bool q = tid & 1;
          auto swap1 = [](const cf v) {     // value of lane ^ 1 (DPP quad_perm [1,0,3,2])
            return make_float2(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v.x), 0xB1, 0xf, 0xf, false)),
                               __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v.y), 0xB1, 0xf, 0xf, false)));
          };
#pragma unroll
          for (int u = 0; u < P::R1 / 2; u++) {
            const cf alo = raw[2 * u].a, ahi = raw[2 * u + 1].a;            // (channel 0, channel 1) of element 2u + q
            const cf aown = q ? ahi : alo, arecv = swap1(q ? alo : ahi);
            raw[2 * u].a = q ? arecv : aown;
            raw[2 * u + 1].a = q ? aown : arecv;
            const cf blo = raw[2 * u].b, bhi = raw[2 * u + 1].b;            // mirror rows: (channel 1, channel 0)
            const cf bown = q ? blo : bhi, brecv = swap1(q ? bhi : blo);
            raw[2 * u].b = q ? brecv : bown;
            raw[2 * u + 1].b = q ? bown : brecv;
          }
          if ((tid >> 1) == 0) raw[0].b = special;
        }
      }
      // MATRIX: x[q] = J[q] (pol0, pol1)[q], Response.C:543-584.  `operand(q)` is what the scalar forms hand to cmuls.  The matrices
      // of element q are the two float4 at rm_at(q) (the bins of load_chirp); group gq + 1 is requested in front of the
      // multiplies of group gq, whose raw[] registers die as its x[] are formed: 64 + 2 * 32 registers live, never more
      // (the schedule barriers keep the scheduler from hoisting all sixteen elements' loads to the top: 128 registers)
      [[maybe_unused]] auto matrix_apply = [&](auto&& operand) {
        constexpr uint32_t MS = 1u << (LOGF - P::LOGR1);
        constexpr int MG = PRESPLIT ? FB_MATRIX_GROUP : FB_MATRIX_GROUP / 2, NMG = PTS / 2 / MG;
        const float4* __restrict__ rm = (const float4*)kernel;
        auto rm_at = [&](const int q) -> const float4* {
          const uint32_t eb = P::G1 * tid + 2 * (q / P::R1);
          return rm + 2 * (((uint64_t)(item.tile * T3 + ((eb & (T - 1)) >> 1)) << LOGF) + (eb >> logT) + (uint32_t)(q % P::R1) * MS);
        };
        float4 f[2][MG][2];
#pragma unroll
        for (int e = 0; e < MG; e++) {
          const float4* __restrict__ p = rm_at(e);
          f[0][e][0] = p[0]; f[0][e][1] = p[1];
        }
#pragma unroll
        for (int gq = 0; gq < NMG; gq++) {
          if (gq + 1 < NMG) {
#pragma unroll
            for (int e = 0; e < MG; e++) {
              const float4* __restrict__ p = rm_at((gq + 1) * MG + e);
              f[(gq + 1) & 1][e][0] = p[0]; f[(gq + 1) & 1][e][1] = p[1];
            }
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int e = 0; e < MG; e++) x[gq * MG + e] = cmatmul(operand(gq * MG + e), f[gq & 1][e][0], f[gq & 1][e][1]);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      // (the uniform real/complex choice is made once, outside the unrolled loops: no branch per element)
      if constexpr (MATRIX) {
        if (PRESPLIT || !g.real_input) {            // (two polarisations always: set_response_matrix refuses npol == 1)
          matrix_apply([&](const int q) { return make_cx2(raw[q].a, raw[q].b); });
        } else {
          matrix_apply([&](const int q) {
            const Abk r = raw[q];
            const cf x0 = make_float2(0.5f * (r.a.x + r.b.x), 0.5f * (r.a.y - r.b.y));
            const cf x1 = make_float2(0.5f * (r.a.y + r.b.y), 0.5f * (r.b.x - r.a.x));
            return make_cx2(x0, x1);
          });
        }
      } else if constexpr (PRESPLIT) {
#pragma unroll
        for (int q = 0; q < PTS / 2; q++) x[q] = cmuls(make_cx2(raw[q].a, raw[q].b), kk[q]);          // Response::operate, Response.C:429-441
      } else if (g.real_input) {
#pragma unroll
        for (int q = 0; q < PTS / 2; q++) {
          const Abk r = raw[q];
          // W[k] = X0[k] + i X1[k] ; conj(W[L-k]) = X0[k] - i X1[k]
          const cf x0 = make_float2(0.5f * (r.a.x + r.b.x), 0.5f * (r.a.y - r.b.y));
          const cf x1 = make_float2(0.5f * (r.a.y + r.b.y), 0.5f * (r.b.x - r.a.x));
          x[q] = cmuls(make_cx2(x0, x1), kk[q]);          // Response::operate, Response.C:429-441
        }
      } else {
        const bool two = g.npol == 2;
#pragma unroll
        for (int q = 0; q < PTS / 2; q++) {
          const Abk r = raw[q];
          x[q] = cmuls(make_cx2(r.a, two ? r.b : make_float2(0.f, 0.f)), kk[q]);
        }
      }
    }
    FB_ST(3, 1);
    const bool more = next_item(++j, next);
    // One burst, and unconditional: the last item of a workgroup is fetched again and dropped.  Under `if (more)` the generic
    // (8-byte) form's loads went to fresh registers and the copies into the loop-carried `raw` sat at the end of the conditional
    // block behind `s_waitcnt vmcnt(16) ... (0)` -- the prefetch was waited for at once (profiles/r04_experiments.txt item 13;
    // what rounds 1-3 read as "the wave time goes to ISSUING the 8-byte loads").  The 16-byte pair form of the headline
    // geometry was not affected.
    fetch(more ? next : item, raw, -1);
    FB_ST(3, 2);

    const uint32_t tile = item.tile;
    const uint64_t part = part0 + item.lp;
    [[maybe_unused]] TsPart tsp = {0, 0, 0, 0};
    [[maybe_unused]] float ts_carry_mid = 0.f;      // SEARCH, two or more stages: the carry of row tid, loaded in mid()
    // COH at freq_res 32 (two stages, 2 T3 threads, 4 T3 rows): the carry of the thread's second row, tid + blockDim.x
    constexpr bool TS_MID2 = COH && FftPlan<LOGF>::NS >= 2 && LOGF < 6;
    [[maybe_unused]] float ts_carry_mid2 = 0.f;
    if constexpr (SEARCH) tsp = ts_part(out, (uint32_t)part, g.nkeep);
    const uint32_t fcs = inv_fold_stride(logT3, g.nkeep, blockDim.x);
    auto chan_of = [&](const uint32_t slo) { return tile * T3 + slo; };
    [[maybe_unused]] uint32_t fcq = 0;              // FOLDQ: samples from one staged channel to the next
    if constexpr (FOLDQ) fcq = inv_foldq_stride(logT3, g.nkeep, blockDim.x, out.prof_planes);
    auto store = [&](const uint32_t col, const uint32_t p, const uint32_t pstride, auto& v) {
      if constexpr (FOLDQ) inv_store_sq(lds, g, out, fcq, g.npol == 2, col, p, pstride, v);
      else inv_store<FOLD, SEARCH, TS_NPO>(lds, g, out, tsp, fcs, chan_of(col >> 1), part, g.npol == 2, col, p, pstride, v);
    };
    // FOLD: this part's active bins, and the accumulator of the thread's first work item (fb_inv_epilogue.h)
    constexpr bool PRE = FOLD && FftPlan<LOGF>::NS >= 2;
    [[maybe_unused]] InvFoldPart fpart = {};
    [[maybe_unused]] InvAcc acc = {};
    [[maybe_unused]] uint4 en_pre[1] = {make_uint4(0, 0, 0, 0)};
    [[maybe_unused]] float4 acc_pre[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
    if constexpr (FOLD) {
      fpart = inv_fold_part(plan, out, jt);
      acc = inv_acc(out, fseg);
    }
    if constexpr (FOLDQ) fpart = inv_fold_part(plan, out, jt);
    auto mid = [&](const int phase) {
      if constexpr (SEARCH) {
        // the open output sample's partial sum (written by this workgroup at the end of the previous part, two barriers ago)
        const uint32_t npo = COH ? 4u : out.state == DSPSR_AMD_PPQQ ? 2u : 1u;
        // (behind the tile's first barrier: that store has been waited for.  Single-stage transforms load theirs behind wgfft: their
        //  mid(1) runs in front of the only barrier that orders the previous tile's carry stores)
        if (FftPlan<LOGF>::NS >= 2 && phase == 2 && tsp.phi && tid < (npo << logT3))
          ts_carry_mid = ts_carry_load(out, (out.chan0 + tile * T3 + tid / npo) * npo + tid % npo);
        if constexpr (TS_MID2) {
          // (the same place in the tile, hence the same order against the previous and this tile's carry stores)
          const uint32_t w = tid + blockDim.x;
          if (phase == 2 && tsp.phi && w < (npo << logT3)) ts_carry_mid2 = ts_carry_load(out, (out.chan0 + tile * T3 + w / npo) * npo + w % npo);
        }
      }
      if constexpr (PRE) {
        if (phase == 2) inv_acc_preload<1>(g, out, acc, fseg, fpart, logT3, tid, blockDim.x, en_pre, acc_pre, chan_of);
        // every wave is past this tile's first exchange barrier, i.e. has left the previous tile's fold: the other plan
        // buffer is free for the entries of the next item
        if (phase == 2 && plan.dma_ok && more) inv_plan_dma(plan, out, walk, next.lp, (jt + 1) & 1, tid);
      }
      if constexpr (FOLDQ && FftPlan<LOGF>::NS >= 2) {       // (the other plan buffer is free, as above; no accumulator is pre-loaded)
        if (phase == 2 && plan.dma_ok && more) inv_plan_dma(plan, out, walk, next.lp, (jt + 1) & 1, tid);
      }
    };
    wgfft<LOGF, +1, EPI != 0>(lds, ltw_off, tid, logT, x, store, mid);
    FB_ST(3, 3);
    if constexpr (SEARCH) {
      const uint32_t npo = COH ? 4u : out.state == DSPSR_AMD_PPQQ ? 2u : 1u, nrow = npo << logT3;
      // the carries of the rows w = tid + k * blockDim.x of this tile (ts_reduce).  nrow / blockDim.x = 16 npo / freq_res
      // (blockDim.x = freq_res * T / 32, nrow = npo * T / 2): one row per thread from freq_res 32 on (two or more stages), up to four
      // below (freq_res 8 with PPQQ; fb_search_fits refuses more).  COH, 64 npo / freq_res = rows per thread: one from freq_res 64 on,
      // two at freq_res 32 (two stages: both loaded in mid), four at freq_res 16 (single stage, below); freq_res 8 is refused
      constexpr int TS_NPRE = FftPlan<LOGF>::NS >= 2 ? (TS_MID2 ? 2 : 1) : 4;
      float ts_carry_pre[TS_NPRE] = {};
      ts_carry_pre[0] = ts_carry_mid;
      if constexpr (TS_MID2) ts_carry_pre[1] = ts_carry_mid2;
      if constexpr (FftPlan<LOGF>::NS < 2) {
        // single stage: behind wgfft's STAGED barrier (the previous tile's carry stores are done) and in front of the barrier
        // below (behind which ts_reduce stores this tile's): all rows of the tile, up to TS_NPRE per thread
        if (tsp.phi) {
#pragma unroll
          for (int k = 0; k < TS_NPRE; k++) {
            const uint32_t w = tid + k * blockDim.x;
            if (w < nrow) ts_carry_pre[k] = ts_carry_load(out, (out.chan0 + tile * T3 + w / npo) * npo + w % npo);
          }
        }
      }
      __syncthreads();                       // the tile's detected samples are staged; every carry of the tile has been read
      ts_reduce<TS_NPO>((const float*)lds, out, tsp, nrow, ts_carry_pre, tid, blockDim.x, chan_of);
      // (the barrier in front of the next tile's first exchange write also ends this read phase)
    }
    if constexpr (FOLD) {
      __syncthreads();                       // the tile's detected samples are staged
      inv_fold_phase<1>(lds, g, out, acc, fseg, fpart, PRE && fpart.in_lds, logT3, fcs, tid, blockDim.x, en_pre, acc_pre, chan_of);
    }
    if constexpr (FOLDQ) {
      __syncthreads();                       // the tile's detected samples are staged
      if (out.prof_planes == 2) inv_foldq_phase<2>(lds, g, out, fseg, fpart, logT3, fcq, tid, blockDim.x, chan_of);
      else inv_foldq_phase<1>(lds, g, out, fseg, fpart, logT3, fcq, tid, blockDim.x, chan_of);
    }
    FB_ST(3, 4);
    FB_ST_TILE(3, 5);
    if (!more) break;
    item = next;
    jt++;
  }
  FB_ST_END(3);
}


}  // namespace dspsr_amd
