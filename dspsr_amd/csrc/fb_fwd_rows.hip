// Convolving filterbank, forward pass 2 (rows of the spectrum); see fb_common.h
#include "fb_common.h"

namespace dspsr_amd {

// ------------------------------------------------------------------------------------ P2
// Rr-point forward FFTs along T2 adjacent rows ka of A (one contiguous block) -> spectrum rows
// s' = kb, bin m = ka, stored as X[s'/T3][m][s'%T3].
// SPLIT (real dual-polarisation input, fb_row_map.h): the T2 rows of the block are T2/2 rows m and their mirrors M - m, so the staged
// tile holds W[m, c] together with W[M - m, Rr - 1 - c] (row 0: W[0, Rr - c], and W[0, 0] for c = 0).  The copy-out forms the
// Hermitian split of every channel c < C = Rr/2 -- the expressions the inverse pass used to evaluate, in the same order -- and
// stores the two polarisations as X'[c/T3][p(m)][c%T3][pol] (p = rm_xrow): as many bytes as X, in aligned runs of (T2/2)*T3 16-byte
// elements.
// (one body, two kernels: k_fwd_rows keeps its name and parameters, k_fwd_rows_split is the SPLIT form)
template <int LOGF, int LOGT, bool SPLIT>
DEV void fwd_rows_body(const FbGeom& g, const cf* __restrict__ A, cf* __restrict__ X, const cf* __restrict__ tw, const uint32_t nparts,
                       const uint32_t nseq, const uint32_t run)
{
  typedef FftPlan<LOGF> P;
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  uint32_t tid = threadIdx.x;
  const int logT = LOGT >= 0 ? LOGT : g.logT2, logT3 = g.logX3;     // X layout block factor
  const uint32_t T2 = 1u << logT, T3 = 1u << logT3;
  const uint64_t L = 1ull << (g.logM + LOGF);
  const uint32_t ntile = 1u << (g.logM - logT);
  const uint32_t total = ntile * nseq * nparts;
  const int logNt = g.logM - logT;          // ntile = 2^logNt
  // The sequences of the launch are walked backwards: the parts written last -- the ones still in the Infinity Cache
  // when the launch ends -- are then the ones the inverse pass, which walks the parts forwards, meets first
  // (+0.8 % Msamples/s in three alternating runs)
  auto seq_of = [&](const uint32_t item) -> uint64_t { return nseq * nparts - 1 - (item >> logNt); };

  // the prefetch keeps the loaded 16-byte pairs untouched (any use would wait for the loads at once);
  // they are rearranged into split form when the tile is started
  auto fetch = [&](const uint32_t item, float4 (&y)[NPAIR]) {
    const uint32_t tile = item & (ntile - 1);
    const cf* __restrict__ Ablk = A + seq_of(item) * L + (((uint64_t)tile << LOGF) << logT);     // g.logR == LOGF
#pragma unroll
    for (int g2 = 0; g2 < P::G1; g2 += 2)
#pragma unroll
      for (int i = 0; i < P::R1; i++)
        y[(g2 / 2) * P::R1 + i] = ld_stream((const float4*)&Ablk[first_stage_elem<LOGF>(tid, logT, g2, i)]);
  };

  const uint32_t ltw_off = lds_pad(PTS * blockDim.x) + 8;      // behind the exchange buffer (16-byte aligned)
  ltw_fill<LOGF>(lds, ltw_off, tw, tid, blockDim.x);
  // copy-out of the staged tile (end of the tile loop): thread part of the addresses, once per kernel
  const uint32_t co_swz = (PTS * blockDim.x) >= 256 ? 3u : 0u;
  const uint32_t co_l0 = 2 * threadIdx.x, co_n2 = LOGT >= 0 ? (2u << (LOGF + LOGT - LOG_PTS)) : 2 * blockDim.x;   // full tiles: a constant
  const int co_sh = logT + logT3;
  const bool co_fast = (co_n2 & 63) == 0 && (g.xblocked || ((co_n2 >> co_sh) != 0 && (co_n2 & ((1u << co_sh) - 1)) == 0));   // uniform
  const uint32_t co_lds = lds_pad(co_l0 ^ (((co_l0 >> 4) & co_swz) << 1)), co_lstep = co_n2 + ((co_n2 >> 6) << 2);
  const uint32_t co_goff = (uint32_t)((g.xblocked ? (uint64_t)co_l0
                                                   : ((((uint64_t)(co_l0 >> co_sh) << g.logM) << logT3) + (co_l0 & ((1u << co_sh) - 1)))) * sizeof(cf));
  const uint64_t co_gstep = g.xblocked ? (uint64_t)co_n2 : (((uint64_t)(co_n2 >> co_sh) << g.logM) << logT3);   // elements of X per pair step
  uint32_t item, next;
  uint32_t j = 0;
  if (!persistent_item(blockIdx.x, gridDim.x, j, run, total, item)) return;
  float4 y[NPAIR];
  fetch(item, y);
  FB_ST_BEGIN(2);
  for (;;) {
    asm volatile("" : "+v"(tid));   // per-tile index math stays inside the loop (see wgfft)
    cx2 x[NPAIR];
    FB_ST(2, 0);                     // (waits for the prefetched tile first)
#pragma unroll
    for (int i = 0; i < NPAIR; i++) x[i] = make_cx2(make_float2(y[i].x, y[i].y), make_float2(y[i].z, y[i].w));
    // The twiddle W_L^{nb*ka} between the two forward passes is applied HERE, to the elements pass 2 has just loaded, not
    // to pass 1's outputs: pass 1 is bound by the vector instructions it issues (31 packed complex products and 10 sin/cos
    // per thread and tile for this twiddle alone), pass 2 by the fabric with its vector unit two thirds idle.  The product
    // nb*ka is symmetric: the column pair is (ka, ka + 1), the position nb = pos0 + i*S.
    {
      const uint32_t tile_t = item & (ntile - 1);
      constexpr uint32_t S = 1u << (LOGF - P::LOGR1);
#pragma unroll
      for (int g2 = 0; g2 < P::G1; g2 += 2) {
        const uint32_t eb = P::G1 * tid + g2;
        cx2 (&xg)[P::R1] = *reinterpret_cast<cx2 (*)[P::R1]>(&x[(g2 / 2) * P::R1]);
        if constexpr (SPLIT) {
          // the column pair is two rows of the mirror-paired block: adjacent in the lower half, descending in the upper one
          const uint32_t r0 = eb & (T2 - 1);
          apply_pass_twiddle2<P::R1>(xg, rm_row(g.logM, logT, tile_t, r0), rm_row(g.logM, logT, tile_t, r0 + 1), eb >> logT, S,
                                     g.logM + LOGF, tw, g.tw_lo);
        } else
        apply_pass_twiddle<P::R1>(xg, tile_t * T2 + (eb & (T2 - 1)), eb >> logT, S, g.logM + LOGF, tw, g.tw_lo);
      }
    }
    FB_ST(2, 1);
    const bool more = persistent_item(blockIdx.x, gridDim.x, ++j, run, total, next);
    if (more) fetch(next, y);
    FB_ST(2, 2);

    const uint32_t tile = item & (ntile - 1);
    cf* __restrict__ Xseq = X + seq_of(item) * g.xstride;
    // last-stage outputs go to LDS in X-layout order [s'/T3][klo][s'%T3]; after a barrier the tile is
    // written out as whole runs of T2*T3 elements with 16-byte-per-lane stores.  XOR swizzle of the image
    // (bits 1,2 ^= bits 4,5) against bank conflicts of the 8-byte scatter (42 % of this pass's LDS cycles)
    const uint32_t swz = (PTS * blockDim.x) >= 256 ? 3u : 0u;
    auto store = [&](const uint32_t klo, const uint32_t p, const uint32_t pstride, auto& v) {
      constexpr int R = sizeof(v) / sizeof(v[0]);
      if constexpr (SPLIT) {
        // the tile as the exchange buffer holds it, element (channel kb, slot r) at lds_pad(kb*T2 + r): a column pair is one
        // 16-byte write, (re, im) of slot klo then of slot klo + 1
#pragma unroll
        for (int k = 0; k < R; k++)
          *(float4*)&lds[lds_pad(((k * pstride + p) << logT) + klo)] = make_float4(v[k].x[0], v[k].y[0], v[k].x[1], v[k].y[1]);
        return;
      }
      auto img = [&](const uint32_t l) { return lds_pad(l ^ (((l >> 4) & swz) << 1)); };
      const uint32_t l0 = ((((p >> logT3) << logT) + klo) << logT3) | (p & (T3 - 1));
      const uint32_t step = pstride << logT;            // image index step per k (pstride is a multiple of T3)
      const bool aff = (step & 63) == 0 && (pstride & (T3 - 1)) == 0;
      const uint32_t b0 = img(l0), b1 = img(l0 + T3), sp = step + (step >> 4);
      if (aff) {                                       // uniform
#pragma unroll
        for (int k = 0; k < R; k++) {
          float* __restrict__ d0 = (float*)&lds[b0 + k * sp];
          float* __restrict__ d1 = (float*)&lds[b1 + k * sp];
          d0[0] = v[k].x[0]; d0[1] = v[k].y[0];
          d1[0] = v[k].x[1]; d1[1] = v[k].y[1];
        }
      } else {
#pragma unroll
        for (int k = 0; k < R; k++) {
          const uint32_t srow = k * pstride + p;
          const uint32_t l = ((((srow >> logT3) << logT) + klo) << logT3) | (srow & (T3 - 1));
          lds[img(l)] = cx2_lo(v[k]);
          lds[img(l + T3)] = cx2_hi(v[k]);
        }
      }
    };
    wgfft<LOGF, -1, true>(lds, ltw_off, tid, logT, x, store);
    __syncthreads();
    FB_ST(2, 3);
    {
      const uint32_t nthr = blockDim.x;
      if constexpr (SPLIT) {
        // 16-byte unit u = tid + jj*nthr of the tile's T2 * C outputs is (channel block cb, row rr, channel clo within the block);
        // rr counts the block's rows in ascending order of m (lower half, then the mirrors from the far end), so that the lanes
        // of a wave write whole runs.  a = W[m, c], b = its mirror; x0 / x1 as in k_inv_chan's unsplit form.
        const uint32_t nth = LOGT >= 0 ? (1u << (LOGF + LOGT - LOG_PTS)) : nthr, Rr = 1u << LOGF, h = T2 >> 1;
        float4* __restrict__ Xs = (float4*)Xseq;
        const bool co_same = (nth & ((1u << (logT + logT3)) - 1)) == 0;     // uniform: only the channel block changes with jj
        uint32_t clo, r, m, rmir;
        auto unit = [&](const uint32_t u) -> uint32_t {
          const uint32_t rr = (u >> logT3) & (T2 - 1);
          clo = u & (T3 - 1);
          r = rr < h ? rr : T2 + h - 1 - rr;
          m = rm_row(g.logM, logT, tile, r);
          rmir = rm_mirror(logT, tile, r);
          return u >> (logT3 + logT);
        };
        uint32_t cb = unit(tid);
        if (co_same && (nth & 63) == 0) {                                    // uniform
          // Unit jj of a thread is unit 0 plus jj channel blocks: channel c0 + jj*(nth/T2), i.e. nth elements further in the
          // image (its mirror nth elements back) and a uniform step further in X' -- two LDS addresses and one 32-bit global
          // offset per thread and tile, the per-unit part an immediate / a scalar.  Computed per unit (64-bit indices, padding,
          // the row map) the copy-out took 4.7k cycles of the tile's 26.5k (profiles/r07_experiments.txt item 3): the two waves
          // of a SIMD issue every vector instruction in four cycles each, and nothing hides them in this phase.
          constexpr uint32_t NU = PTS / 2;
          const uint32_t c0 = (cb << logT3) | clo, lstep = nth + (nth >> 4);
          const uint32_t cm0 = m ? Rr - 1 - c0 : Rr - c0;                    // mirror channel (row 0: Rr - c; c = 0 is its own, see lb0)
          const uint32_t la = lds_pad((c0 << logT) + r);
          const uint32_t lb = lds_pad((cm0 << logT) + rmir - (NU - 1) * nth);   // mirror of unit jj at lb + (NU - 1 - jj)*lstep  (cm0 >= 31 nth / T2)
          const uint32_t lb0 = (m == 0 && c0 == 0) ? lds_pad(rmir) : lb + (NU - 1) * lstep;
          // (bytes within the sequence: 16 C M = 8 L <= 2^29)
          const uint32_t goff = (uint32_t)rm_xsplit_index(g.logM, logT3, c0, m) * (uint32_t)sizeof(float4);
          const uint64_t gstep = ((uint64_t)(nth >> (logT3 + logT)) << (g.logM + logT3)) * sizeof(float4);
          const char* __restrict__ gb = (const char*)Xs;
#pragma unroll
          for (int j4 = 0; j4 < PTS / 2; j4 += 4) {
            cf a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
              a[q] = lds[la + (j4 + q) * lstep];
              b[q] = lds[j4 + q == 0 ? lb0 : lb + (NU - 1 - (j4 + q)) * lstep];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const cf x0 = make_float2(0.5f * (a[q].x + b[q].x), 0.5f * (a[q].y - b[q].y));
              const cf x1 = make_float2(0.5f * (a[q].y + b[q].y), 0.5f * (b[q].x - a[q].x));
              st_stream((float4*)(gb + (uint64_t)(j4 + q) * gstep + goff), make_float4(x0.x, x0.y, x1.x, x1.y));
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
#pragma unroll
        for (int j4 = 0; j4 < PTS / 2; j4 += 4) {
          cf a[4], b[4];
          uint64_t gi[4];
#pragma unroll
          for (int q = 0; q < 4; q++) {
            if (j4 + q) cb = co_same ? cb + (nth >> (logT3 + logT)) : unit(tid + (j4 + q) * nth);
            const uint32_t c = (cb << logT3) | clo;
            const uint32_t cm = m ? Rr - 1 - c : (Rr - c) & (Rr - 1);
            a[q] = lds[lds_pad((c << logT) + r)];
            b[q] = lds[lds_pad((cm << logT) + rmir)];
            gi[q] = rm_xsplit_index(g.logM, logT3, c, m);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < 4; q++) {
            // W[k] = X0[k] + i X1[k] ; conj(W[L-k]) = X0[k] - i X1[k]
            const cf x0 = make_float2(0.5f * (a[q].x + b[q].x), 0.5f * (a[q].y - b[q].y));
            const cf x1 = make_float2(0.5f * (a[q].y + b[q].y), 0.5f * (b[q].x - a[q].x));
            st_stream(&Xs[gi[q]], make_float4(x0.x, x0.y, x1.x, x1.y));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        }
      } else
      if (co_fast) {
        // thread part of the addresses computed once per kernel, per-pair part an immediate / a uniform step (see pass 1)
        const char* __restrict__ gb = (const char*)(Xseq + (g.xblocked ? (uint64_t)tile * g.xblock : ((uint64_t)(tile * T2) << logT3)));
#pragma unroll
        for (int j4 = 0; j4 < PTS / 2; j4 += 4) {
          float4 pr[4];
#pragma unroll
          for (int q = 0; q < 4; q++) pr[q] = *(const float4*)&lds[co_lds + (j4 + q) * co_lstep];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < 4; q++) st_stream((float4*)(gb + (uint64_t)(j4 + q) * co_gstep * sizeof(cf) + co_goff), pr[q]);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll 4
        for (int jj = 0; jj < PTS / 2; jj++) {
          const uint32_t l = 2 * (tid + jj * nthr);
          const uint32_t blkX = l >> (logT + logT3), within = l & ((1u << (logT + logT3)) - 1);
          const float4 pr = *(const float4*)&lds[lds_pad(l ^ (((l >> 4) & swz) << 1))];
          // four-pass mode (xblocked): the tile's image [kb][ka % T2] IS its block of X -- one contiguous 2^14-element
          // store instead of runs of T2 elements scattered over the natural order
          const uint64_t xo = g.xblocked ? (uint64_t)tile * g.xblock + l
                                         : ((((uint64_t)blkX << g.logM) + tile * T2) << logT3) + within;
          st_stream((float4*)&Xseq[xo], pr);
        }
      }
    }
    FB_ST(2, 4);
    FB_ST_TILE(2, 5);
    if (!more) break;
    item = next;
  }
  FB_ST_END(2);
}

template <int LOGF, int LOGT>
__global__ __launch_bounds__(512) void k_fwd_rows(const FbGeom g, const cf* __restrict__ A, cf* __restrict__ X,
                                                  const cf* __restrict__ tw, const uint32_t nparts,
                                                  const uint32_t nseq, const uint32_t run)
{
  fwd_rows_body<LOGF, LOGT, false>(g, A, X, tw, nparts, nseq, run);
}
template <int LOGF, int LOGT>
__global__ __launch_bounds__(512) void k_fwd_rows_split(const FbGeom g, const cf* __restrict__ A, cf* __restrict__ X,
                                                        const cf* __restrict__ tw, const uint32_t nparts,
                                                        const uint32_t nseq, const uint32_t run)
{
  fwd_rows_body<LOGF, LOGT, true>(g, A, X, tw, nparts, nseq, run);
}


template <int... I> static k2_t pick2(int logf, bool full, bool presplit, iseq<I...>)
{
  static const k2_t t[] = {k_fwd_rows<I, -1>...};
  static const k2_t f[] = {k_fwd_rows<I, full_logt(I)>...};
  static const k2_t ts[] = {k_fwd_rows_split<I, -1>...};
  static const k2_t fs[] = {k_fwd_rows_split<I, full_logt(I)>...};
  return presplit ? (full ? fs[logf] : ts[logf]) : (full ? f[logf] : t[logf]);
}
k2_t fb_pick2(int logf, bool full, bool presplit) { return pick2(logf, full, presplit, seq_t()); }

}  // namespace dspsr_amd

FB_ST_READER(fwd_rows)
