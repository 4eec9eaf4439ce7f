// The transform-detect tile shared by k_plfb (plfb.hip) and k_bandpass (bandpass.hip): transform a tile of (part, polarisation)
// columns, detect every bin, add the products to register sums.
//
// A workgroup tile is wgfft's 16384 points: C complex points x T = 16384 / C columns, the columns being the (part, polarisation)
// pairs of Tp = T / 2 parts -- both polarisations of a part are the two halves of a thread's butterfly pair, as in k_tfp.  Nyquist
// rows are transformed as C complex points z[n] = x[2n] + i x[2n+1] followed by the Hermitian split (k_tfp's), never as a 2 C point
// transform.  The transform is staged in the exchange buffer, one plane of C float4 (Re p0, Re p1, Im p0, Im p1) per part; thread t
// then owns bins t, t + 512, ... (bin pairs (k, C - k) for Nyquist rows, 0 paired with C / 2) of EVERY part of the tile.
//
// What a kernel brings: how an element of a part is loaded (transform's `load`), when the sums leave the registers and where they
// go (for_owned's `f`), and the two parameters below.  The statements are the two kernels' own, moved: the library is built with
// -ffp-contract=on, which contracts within a statement, and tests/test_gpu_spectral_sums_parent.py compares bits.
#pragma once
#include "wgfft.h"

namespace dspsr_amd {

constexpr uint32_t ST_THREADS = 512;

// SUM_POL: with NPO == 1, add p0 + p1 (two input polarisations give total intensity) and not p0 alone (npol_out == npol_in).
// HOLD_NB: the Nyquist twiddles are held in registers across the tiles where a thread owns at most this many bin pairs, and
// evaluated per use -- the same instructions on the same argument, the same bits -- above it.
template <int LOGC, int NDIM, int NPO, bool SUM_POL, int HOLD_NB>
struct SpectralTile {
  typedef FftPlan<LOGC> P;
  static constexpr uint32_t nt = ST_THREADS;
  static constexpr int logT = 14 - LOGC, logTp = logT - 1;
  static constexpr uint32_t Tp = 1u << logTp, C = 1u << LOGC;
  static constexpr uint32_t NK = NDIM == 2 ? C : C / 2;     // bins (Analytic) or bin pairs (Nyquist) of a part
  static constexpr int NB = NK > nt ? NK / nt : 1;          //   ... of which a thread owns NB
  static constexpr int NE = NDIM == 2 ? 1 : 2;
  static constexpr bool HOLD_W = NB <= HOLD_NB;
  static constexpr uint32_t plane = C + (Tp <= 64 ? 8u : 0u);
  typedef float Acc[NB][NE][NPO];
  typedef float Tw[HOLD_W ? NB : 1];

  // wgfft's twiddle table into LDS; its offset
  static DEV uint32_t fill_twiddle_table(cf* lds, const cf* __restrict__ tw, const uint32_t tid)
  {
    const uint32_t ltw_off = lds_pad(PTS * nt) + 8;
    ltw_fill<LOGC>(lds, ltw_off, tw, tid, nt);
    return ltw_off;
  }

  // Nyquist: w^k = exp(-i pi k / C) = (wcos, -wsin), argument k / 2C revolutions, exact in float
  static DEV float wcos(const uint32_t k) { return __builtin_amdgcn_cosf((float)k * __uint_as_float((uint32_t)(127 - (LOGC + 1)) << 23)); }
  static DEV float wsin(const uint32_t k) { return __builtin_amdgcn_sinf((float)k * __uint_as_float((uint32_t)(127 - (LOGC + 1)) << 23)); }
  static DEV void twiddles(Tw& wc, Tw& ws)
  {
    if constexpr (HOLD_W) {
#pragma unroll
      for (int j = 0; j < NB; j++) {
        wc[j] = wcos(threadIdx.x + j * nt);
        ws[j] = wsin(threadIdx.x + j * nt);
      }
    }
  }

  static DEV void zero(Acc& acc)
  {
#pragma unroll
    for (int j = 0; j < NB; j++)
#pragma unroll
      for (int e = 0; e < NE; e++)
#pragma unroll
        for (int q = 0; q < NPO; q++) acc[j][e][q] = 0.f;
  }

  // the detected products of one bin: (re, im) of the two polarisations (PhaseLockedFilterbank.C:275-276, :288-293; Response.C:484-489,
  // cross_detect.ic:39-40)
  static DEV void detect(float (&s)[NPO], const float r0, const float i0, const float r1, const float i1, const float sgn)
  {
    float p0 = r0 * r0; p0 += i0 * i0;
    if constexpr (NPO == 1 && !SUM_POL) {
      s[0] += p0;
    } else {
      float p1 = r1 * r1; p1 += i1 * i1;
      if constexpr (NPO == 1) {
        s[0] += p0 + p1;
      } else {
        s[0] += p0;
        s[1] += p1;
        if constexpr (NPO == 4) {
          s[2] += r0 * r1 + i0 * i1;
          s[NPO == 4 ? 3 : 0] += sgn * (r0 * i1 - i0 * r1);
        }
      }
    }
  }

  // The staged transform of the tile whose first part is w0: load(w, n, v0, v1) fills polarisation 0 and 1 of complex element n of
  // part w < w_end (parts from w_end on, and what load leaves alone, are zero).  Ends behind the barrier: the planes can be read.
  // tid is made opaque here, once per tile, so that the addresses formed from it stay inside the tile loop.  k_bandpass hands over
  // its own variable, as it always did; k_plfb hands over a copy per tile (on its own variable k_plfb<13, 1, 4> spills 8 bytes).
  template <class Load>
  static DEV void transform(cf* lds, const uint32_t ltw_off, uint32_t& tid, const uint32_t w0, const uint32_t w_end, Load load)
  {
    asm volatile("" : "+v"(tid));
    cx2 x[NPAIR];
#pragma unroll
    for (int g2 = 0; g2 < P::G1; g2 += 2)
#pragma unroll
      for (int i = 0; i < P::R1; i++) {
        const uint32_t el = first_stage_elem<LOGC>(tid, logT, g2, i);
        const uint32_t w = w0 + ((el & ((1u << logT) - 1)) >> 1), n = el >> logT;
        float2 v0 = make_float2(0.f, 0.f), v1 = make_float2(0.f, 0.f);
        if (w < w_end) load(w, n, v0, v1);
        cx2& d = x[(g2 / 2) * P::R1 + i];
        d.x = (v2f){v0.x, v1.x};
        d.y = (v2f){v0.y, v1.y};
      }
    float4* const stg = (float4*)lds;                       // k_tfp's staging
    auto store = [&](const uint32_t col, const uint32_t pp, const uint32_t pstride, auto& v) {
      constexpr int R = sizeof(v) / sizeof(v[0]);
      float4* const d = stg + (col >> 1) * plane + pp;
#pragma unroll
      for (int k = 0; k < R; k++) d[k * pstride] = make_float4(v[k].x[0], v[k].x[1], v[k].y[0], v[k].y[1]);
    };
    wgfft<LOGC, -1, true>(lds, ltw_off, tid, logT, x, store);
    __syncthreads();
  }

  // adds the detected bins this thread owns of staged part c2 of the tile; the caller's barrier follows the tile's last part (the
  // next tile's exchanges overwrite the staged image)
  static DEV void add_part(Acc& acc, const cf* lds, const uint32_t c2, const Tw& wc, const Tw& ws)
  {
    const float4* const pl = (const float4*)lds + c2 * plane;
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
        // (k comes from the opaque t0: an evaluation stays inside the loop)
        const float c = HOLD_W ? wc[HOLD_W ? j : 0] : wcos(k), sn = HOLD_W ? ws[HOLD_W ? j : 0] : wsin(k);
        const v2f wr = c * br + sn * bi, wi = c * bi - sn * br;
        const v2f xr = ar + wr, xi = ai + wi;
        detect(acc[j][0], xr[0], xi[0], xr[1], xi[1], 1.f);
        if (k) {
          const v2f yr = ar - wr, yi = ai - wi;             // X[C-k] = (yr, -yi)
          detect(acc[j][NE - 1], yr[0], yi[0], yr[1], yi[1], -1.f);
        } else {
          const float4 zh = pl[C / 2];                      // X[C/2] = (Re Z, -Im Z)
          detect(acc[j][NE - 1], zh.x, zh.z, zh.y, zh.w, -1.f);
        }
      }
    }
  }

  // f(j, e, bin) for every sum acc[j][e] this thread owns: bin k, and for Nyquist rows its mirror C - k (0 is paired with C / 2)
  template <class F>
  static DEV void for_owned(F f)
  {
    uint32_t t0 = threadIdx.x;
    asm volatile("" : "+v"(t0));                            // (loop-invariant addresses: keep them out of the tile loop's registers)
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const uint32_t k = t0 + j * nt;
      if (k >= NK) continue;
#pragma unroll
      for (int e = 0; e < NE; e++) f(j, e, e == 0 ? k : (k ? C - k : C / 2));
    }
  }
};

}  // namespace dspsr_amd
