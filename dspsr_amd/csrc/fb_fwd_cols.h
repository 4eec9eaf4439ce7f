// Convolving filterbank, forward pass 1 (k_fwd_cols); instantiated by fb_fwd_cols.hip (rows of A in natural order) and
// fb_fwd_cols_rm.hip (mirror-paired row order, fb_row_map.h): two translation units so that the two families compile in parallel.
#pragma once
#include "fb_common.h"

namespace dspsr_amd {

// ------------------------------------------------------------------------------------ P1
// M-point forward FFTs down T1 adjacent stride-Rr columns of one sequence of one part.
//   in : sample n = na*Rr + nb (8-bit or float32, converted on load), nb = tile*T1 + col
//   out: A[ka/T2][nb][ka%T2] = W_L^{nb*ka} * sum_na w[na*Rr+nb] W_M^{na*ka}
// Persistent: each workgroup walks its items (tile fastest, then sequence, then part) and
// prefetches the raw samples of the next item while transforming the current one.
// LOGT >= 0: the number of columns per tile (2^LOGT) is a compile-time constant (the usual full-size tile,
// LOGT = 14 - LOGF), so every LDS address and stride folds into immediates; LOGT = -1: taken from the geometry.
// RMAP: the rows ka of A in the mirror-paired order of fb_row_map.h (block, slot) instead of (ka / T2, ka % T2); only the place of
// a row in the staged image changes, the copy-out and its runs do not.
// (one body, two kernels: k_fwd_cols keeps its name and parameters, k_fwd_cols_rm is the RMAP form)
template <int LOGF, int RAWW, int LOGT, bool RMAP>
DEV void fwd_cols_body(const FbGeom& g, const FbIn& in, cf* __restrict__ A, const cf* __restrict__ tw, const uint64_t part0,
                       const uint32_t nparts, const uint32_t nseq, const uint32_t run)
{
  typedef FftPlan<LOGF> P;
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  uint32_t tid = threadIdx.x;
  const int logT = LOGT >= 0 ? LOGT : g.logT1, logT2 = g.logT2;
  const uint32_t T = 1u << logT, T2 = 1u << logT2;
  const int logL = LOGF + g.logR;          // g.logM == LOGF
  const uint64_t L = 1ull << logL;
  const uint32_t ntile = 1u << (g.logR - logT);
  const uint32_t total = ntile * nseq * nparts;
  const int logNt = g.logR - logT;          // ntile = 2^logNt ; nseq is 1 or 2
  auto seq_of = [&](const uint32_t rest) { return nseq == 2 ? (rest & 1u) : 0u; };
  auto part_of = [&](const uint32_t rest) { return nseq == 2 ? (rest >> 1) : rest; };

  auto fetch = [&](const uint32_t item, RawW<RAWW> (&raw)[PTS / 2]) {
    const uint32_t tile = item & (ntile - 1);
    const uint32_t rest = item >> logNt;
    uint32_t seq = seq_of(rest);
    const bool pret = in.kind == FB_IN_RT_BYTES || in.kind == FB_IN_RT_FLOAT;   // pre-transposed: [na][T] pairs, contiguous per tile (fb_rt_layout.h)
    uint64_t t0 = pret ? part_of(rest) * in.rt_part_stride + seq * in.rt_seq_stride + tile * in.rt_tile_stride
                       : (part0 + part_of(rest)) * in.part_step + tile * T;
    if constexpr (RAWW == 4) {
      // channel-batched convolution (FbIn::batch, float32 complex rows): `rest` = (part * npol + pol) * batch + channel
      if (in.batch) {                                  // uniform
        const uint32_t c = rest % in.batch, ps = rest / in.batch;
        seq = ps % (uint32_t)g.npol;
        t0 = (part0 + ps / (uint32_t)g.npol) * in.part_step + c * in.chan_stride_c + tile * T;
      }
    }
    // element i of a thread's first-stage butterfly is row na = nab + i*MS of one column pair: sample index =
    // base + i*step with a wave-uniform step (no per-element index arithmetic or branches between the loads)
    constexpr uint32_t MS = 1u << (LOGF - P::LOGR1);
    const uint64_t step = pret ? ((uint64_t)MS << logT) : ((uint64_t)MS << g.logR);
#pragma unroll
    for (int g2 = 0; g2 < P::G1; g2 += 2) {
      const uint32_t eb = P::G1 * tid + g2;               // element of the tile: row eb >> logT, column eb % T
      const uint64_t tb = t0 + (eb & (T - 1)) + (pret ? (uint64_t)((eb >> logT) << logT) : (((uint64_t)(eb >> logT)) << g.logR));
#pragma unroll
      for (int i = 0; i < P::R1; i++) raw[(g2 / 2) * P::R1 + i] = fetch_pair<RAWW>(g, in, seq, tb + i * step);
    }
  };

  // exchange buffer, then the stage twiddle tables (16-byte aligned)
  const uint32_t ltw_off = lds_pad(PTS * blockDim.x) + 8;
  ltw_fill<LOGF>(lds, ltw_off, tw, threadIdx.x, blockDim.x);
  // copy-out of the staged tile (see the end of the tile loop): thread part of the addresses, once per kernel
  const uint32_t co_swz = (PTS * blockDim.x) >= 256 ? 1u : 0u;
  const uint32_t co_l0 = 2 * threadIdx.x;
  const uint32_t co_n2 = LOGT >= 0 ? (2u << (LOGF + LOGT - LOG_PTS)) : 2 * blockDim.x;   // full tiles: a constant
  const int co_sh = logT + logT2;
  const bool co_fast = (co_n2 & 63) == 0 && (co_n2 >> co_sh) != 0 && (co_n2 & ((1u << co_sh) - 1)) == 0;   // uniform
  const uint32_t co_lds = lds_pad(co_l0 ^ (((co_l0 >> 4) & co_swz) << 3)), co_lstep = co_n2 + ((co_n2 >> 6) << 2);
  const uint32_t co_goff = (uint32_t)(((((uint64_t)(co_l0 >> co_sh) << g.logR) << logT2) + (co_l0 & ((1u << co_sh) - 1))) * sizeof(cf));
  const uint64_t co_gstep = ((uint64_t)(co_n2 >> co_sh) << g.logR) << logT2;       // elements of A per pair step
  auto copy_out = [&](const uint32_t tile, cf* __restrict__ Aseq) {
    const uint32_t swz = co_swz;
    const uint32_t nthr = blockDim.x;
    if (co_fast) {
      // pair jj of a thread is pair 0 plus jj*2*nthr elements: a constant step in the padded image (co_lstep) and a
      // uniform step in A (co_gstep) -- one LDS address and one 32-bit global offset per THREAD, computed before the
      // tile loop; the per-pair part is an immediate / a scalar-register base (this loop issued 23 % of the pass's
      // vector instructions as per-pair address arithmetic, 64-bit shifts included)
      const char* __restrict__ gb = (const char*)(Aseq + ((uint64_t)(tile * T) << logT2));
#pragma unroll
      for (int j4 = 0; j4 < PTS / 2; j4 += 4) {                  // four LDS reads in flight, then their stores
        float4 pr[4];
#pragma unroll
        for (int q = 0; q < 4; q++) pr[q] = *(const float4*)&lds[co_lds + (j4 + q) * co_lstep];
        __builtin_amdgcn_sched_barrier(0);                         // (the min-register scheduler would pair every read with its store)
#pragma unroll
        for (int q = 0; q < 4; q++) st_stream((float4*)(gb + (uint64_t)(j4 + q) * co_gstep * sizeof(cf) + co_goff), pr[q]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll 4
      for (int jj = 0; jj < PTS / 2; jj++) {
        const uint32_t l = 2 * (tid + jj * nthr);                  // element index inside the staged image
        const uint32_t blkA = l >> (logT + logT2), within = l & ((1u << (logT + logT2)) - 1);
        const float4 pr = *(const float4*)&lds[lds_pad(l ^ (((l >> 4) & swz) << 3))];
        st_stream((float4*)&Aseq[((((uint64_t)blkA << g.logR) + tile * T) << logT2) + within], pr);
      }
    }
  };
  uint32_t item, next;
  uint32_t j = 0;
  if (!persistent_item(blockIdx.x, gridDim.x, j, run, total, item)) return;
  RawW<RAWW> raw[PTS / 2];
  fetch(item, raw);
  FB_ST_BEGIN(1);
  for (;;) {
    asm volatile("" : "+v"(tid));   // per-tile index math stays inside the loop (see wgfft)
    cx2 x[NPAIR];
    FB_ST(1, 0);                     // (waits for the prefetched tile first)
    const uint32_t seq_cur = seq_of(item >> logNt);
#pragma unroll
    for (int h = 0; h < NPAIR; h++) {
      cf a, b;
      decode_pair<RAWW>(g, in, raw[h], a, b, seq_cur);
      x[h] = make_cx2(a, b);
    }
    FB_ST(1, 1);
    const bool more = persistent_item(blockIdx.x, gridDim.x, ++j, run, total, next);
    if (more) fetch(next, raw);
    FB_ST(1, 2);

    const uint32_t tile = item & (ntile - 1);
    cf* __restrict__ Aseq = A + (uint64_t)(item >> logNt) * L;                 // sequence part*nseq + seq
    // last-stage outputs go to LDS in A-layout order [ka/T2][col][ka%T2]; after a barrier the tile is
    // written out as whole runs of T*T2 elements with 16-byte-per-lane stores.  The image is XOR-swizzled
    // (bit 3 ^= bit 4; pairs of elements stay together) so that the 8-byte scatter of a wave spreads over all
    // banks (17 % of this pass's LDS cycles were bank conflicts, profiles/r01d_lds_conflicts.txt).
    // (the twiddle W_L^{nb*ka} between the two forward passes is applied by pass 2, on load: see k_fwd_rows)
    const uint32_t swz = (PTS * blockDim.x) >= 256 ? 1u : 0u;
    auto store = [&](const uint32_t col, const uint32_t p, const uint32_t pstride, auto& v) {
      constexpr int R = sizeof(v) / sizeof(v[0]);
      // image index of element k: l0 + k*(pstride << logT) (pstride is a multiple of T2), so when that step is a
      // multiple of 64 the swizzle and the padding of l0 carry over: one address per column, constant offsets
      auto img = [&](const uint32_t l) { return lds_pad(l ^ (((l >> 4) & swz) << 3)); };
      if constexpr (RMAP) {
        // Mirror-paired row order (fb_row_map.h): row ka in slot (block, r) lies at image index ((block << logT) + col) << logT2 | r.
        // v[k] is row ka = k*pstride + p and R*pstride = M, so k < R/2 are the rows below M/2 and, with pstride a multiple of T2,
        // their block grows by 2*pstride/T2 per k while the slot stays.  The rows above M/2 are the mirrors of
        // M - ka = (R-1-k)*pstride + (pstride - p): the same step, walked from k = R-1 downwards.  p = 0: M - ka = (R-k)*pstride,
        // and row M/2 (k = R/2) has the slot the mirror of row 0 would have.
        auto idx = [&](const RowSlot s) { return (((s.block << logT) + col) << logT2) | s.r; };
        constexpr int LM = LOGF >= 1 ? LOGF : 1;           // (LOGF = 0 is instantiated, never launched in this form)
        constexpr uint32_t Mr = 1u << LM;
        const uint32_t step = pstride << (logT + 1);
        const bool aff = R >= 2 && (step & 63) == 0 && (pstride & (T2 - 1)) == 0;
        if (aff) {                                     // uniform
          const uint32_t sp = step + (step >> 4);
          const uint32_t l0 = idx(rm_slot(LM, logT2, p));
          const uint32_t l1 = idx(rm_slot(LM, logT2, p ? Mr - (pstride - p) : Mr >> 1));
          const uint32_t b0 = img(l0), b1 = img(l0 + T2), h0 = img(l1), h1 = img(l1 + T2);
          // upper rows k > R/2 at u + (R-1-k)*sp; k = R/2 at m
          const uint32_t u0 = p ? h0 : h0 + sp, u1 = p ? h1 : h1 + sp;
          const uint32_t m0 = p ? h0 + (R / 2 - 1) * sp : h0, m1 = p ? h1 + (R / 2 - 1) * sp : h1;
#pragma unroll
          for (int k = 0; k < R; k++) {
            float* __restrict__ d0 = (float*)&lds[k < R / 2 ? b0 + k * sp : k == R / 2 ? m0 : u0 + (R - 1 - k) * sp];
            float* __restrict__ d1 = (float*)&lds[k < R / 2 ? b1 + k * sp : k == R / 2 ? m1 : u1 + (R - 1 - k) * sp];
            d0[0] = v[k].x[0]; d0[1] = v[k].y[0];
            d1[0] = v[k].x[1]; d1[1] = v[k].y[1];
          }
        } else {
#pragma unroll
          for (int k = 0; k < R; k++) {
            const uint32_t l = idx(rm_slot(LM, logT2, k * pstride + p));
            lds[img(l)] = cx2_lo(v[k]);
            lds[img(l + T2)] = cx2_hi(v[k]);
          }
        }
        return;
      }
      const uint32_t l0 = ((((p >> logT2) << logT) + col) << logT2) | (p & (T2 - 1));
      const uint32_t step = pstride << logT;
      const bool aff = (step & 63) == 0 && (pstride & (T2 - 1)) == 0;
      const uint32_t b0 = img(l0), b1 = img(l0 + T2), sp = step + (step >> 4);
      if (aff) {                                       // uniform
#pragma unroll
        for (int k = 0; k < R; k++) {
          float* __restrict__ d0 = (float*)&lds[b0 + k * sp];
          float* __restrict__ d1 = (float*)&lds[b1 + k * sp];
          d0[0] = v[k].x[0]; d0[1] = v[k].y[0];       // (re, im) of column col   (two dwords: no register shuffling)
          d1[0] = v[k].x[1]; d1[1] = v[k].y[1];       // column col + 1
        }
      } else {
#pragma unroll
        for (int k = 0; k < R; k++) {
          const uint32_t ka = k * pstride + p;
          const uint32_t l = ((((ka >> logT2) << logT) + col) << logT2) | (ka & (T2 - 1));
          lds[img(l)] = cx2_lo(v[k]);
          lds[img(l + T2)] = cx2_hi(v[k]);
        }
      }
    };
    wgfft<LOGF, -1, true>(lds, ltw_off, tid, logT, x, store);
    __syncthreads();
    FB_ST(1, 3);
    copy_out(tile, Aseq);
    FB_ST(1, 4);
    FB_ST_TILE(1, 5);
    if (!more) break;
    item = next;
  }
  FB_ST_END(1);
}

template <int LOGF, int RAWW, int LOGT>
__global__ __launch_bounds__(512) void k_fwd_cols(const FbGeom g, const FbIn in, cf* __restrict__ A,
                                                  const cf* __restrict__ tw, const uint64_t part0,
                                                  const uint32_t nparts, const uint32_t nseq, const uint32_t run)
{
  fwd_cols_body<LOGF, RAWW, LOGT, false>(g, in, A, tw, part0, nparts, nseq, run);
}
template <int LOGF, int RAWW, int LOGT>
__global__ __launch_bounds__(512) void k_fwd_cols_rm(const FbGeom g, const FbIn in, cf* __restrict__ A,
                                                     const cf* __restrict__ tw, const uint64_t part0,
                                                     const uint32_t nparts, const uint32_t nseq, const uint32_t run)
{
  fwd_cols_body<LOGF, RAWW, LOGT, true>(g, in, A, tw, part0, nparts, nseq, run);
}

}  // namespace dspsr_amd
