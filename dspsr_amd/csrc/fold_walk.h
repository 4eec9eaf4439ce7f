// What the chunk kernels of fold.hip share (k_fold_chunked, k_fold_dense, k_fold_many), each piece once: the chunk stream (global
// memory -> registers -> the chunk image in LDS), the cursor of one owned phase bin into its time-ordered interval list, the split
// of a LONG run piece, the dense table entry, the run add from the chunk image, and the store of an owned bin's accumulators.
// Everything is force-inlined into the kernel that calls it and takes its scalars by value.  The chunk image is handed over as
// the kernel's __shared__ array itself: once inlined the compiler sees the LDS address space and the reads are ds_read (a pointer
// it cannot resolve would turn them into flat loads whose vmcnt(0) wait also drains the chunk prefetch; checked in the
// disassembly, profiles/HISTORY.md).  k_fold_moments (fold_moments.hip) is the same machine with loaders of its own; it takes the
// LONG piece split from here and keeps its own cursor, which as FoldCursor cost its stream loader a quarter of its speed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fold_plan.h"

namespace dspsr_amd {

// The chunk image of the FOLD_CHUNK-sample kernels: NROW rows of RS floats, fetched as NF4 float4 per row, at most MAXR of them
// per thread (256 threads at least); LONG adds MS micro-block sums per row.
template <int NDIM>
struct FoldImage {
  static constexpr uint32_t RS = FOLD_CHUNK * NDIM;
  static constexpr uint32_t NF4 = RS / 4;
  static constexpr uint32_t MAXR = NF4 / 256;
  static constexpr uint32_t MS = (FOLD_CHUNK / FOLD_MB) * NDIM;
};

// ---- chunk stream ----------------------------------------------------------------------------------------------------------------
// Chunk c (NF4 float4 per row, rows pol_stride floats apart from src0, the first sample of the span; 16-byte aligned: the host
// sends other rows to k_fold_direct) into pre[][]: thread tid of nt takes float4 tid, tid + nt, ...  Of the span's nfl_total floats
// nothing behind the last is read: the ragged end is filled float by float, zeros behind it.
template <uint32_t NF4, int NROW, uint32_t MAXR>
static __device__ __forceinline__ void fold_fetch(float4 (&pre)[NROW][MAXR], const float* src0, const uint64_t pol_stride,
                                                  const uint64_t nfl_total, const uint32_t c, const uint32_t tid, const uint32_t nt)
{
#pragma unroll
  for (int rw = 0; rw < NROW; rw++) {
    const float4* src = (const float4*)(src0 + rw * pol_stride);
#pragma unroll
    for (uint32_t r = 0; r < MAXR; r++) {
      const uint32_t q = tid + r * nt;
      const uint64_t k = (uint64_t)c * NF4 + q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < NF4) {
        if (4 * k + 4 <= nfl_total) {
          v = src[k];
        } else if (4 * k < nfl_total) {                  // ragged end of the span: never read past it
          const float* t = (const float*)(src + k);
          const uint32_t n = (uint32_t)(nfl_total - 4 * k);
          v.x = t[0];
          if (n > 1) v.y = t[1];
          if (n > 2) v.z = t[2];
        }
      }
      pre[rw][r] = v;
    }
  }
}

// pre[][] into the chunk image (between the two barriers of a chunk)
template <uint32_t NF4, int NROW, uint32_t MAXR>
static __device__ __forceinline__ void fold_store(float* lds, const float4 (&pre)[NROW][MAXR], const uint32_t tid, const uint32_t nt)
{
#pragma unroll
  for (int rw = 0; rw < NROW; rw++)
#pragma unroll
    for (uint32_t r = 0; r < MAXR; r++)
      if (tid + r * nt < NF4) ((float4*)(lds + rw * (4 * NF4)))[tid + r * nt] = pre[rw][r];
}

// ---- interval cursor of one owned bin --------------------------------------------------------------------------------------------
// Plan pointers are template parameters: `const Interval*` / `const uint32_t*` where they are kernel arguments; k_fold_many reads
// its plans' pointers from LDS, where they are generic, and casts them to the global address space (fold.hip GlobalIv).
// "no interval" = offset ~0.  Always a load through the plan pointer with a clamped index: selecting between &iv[i] and a local
// would make the load generic (flat_load + full vmcnt/lgkmcnt drain).
template <class IvPtr>
static __device__ __forceinline__ void fold_load_iv(const IvPtr iv, const uint32_t i, const bool valid, uint64_t& offset, uint32_t& hits)
{
  const IvPtr p = iv + (valid ? i : 0u);
  offset = p->offset;
  hits = p->hits;
  if (!valid) { offset = ~0ull; hits = 0u; }
}

// The current and the following interval are kept in registers (loaded long before they are needed) so the chunk loop never
// waits on global memory.
struct FoldCursor {
  uint32_t cur, end;
  uint64_t off0, off1;   // first sample of the current interval, of the following one
  uint32_t hits0, hits1;

  // bin b of the plan (owned: the thread has one); SEEK: start at the first interval that reaches behind sample seg0 (LONG time
  // segments; intervals are time ordered: binary search)
  template <bool SEEK, class StartPtr, class IvPtr>
  __device__ __forceinline__ void open(const StartPtr bin_start, const IvPtr iv, const uint32_t b, const bool owned, const uint64_t seg0)
  {
    cur = end = 0;
    if (owned) { cur = bin_start[b]; end = bin_start[b + 1]; }
    if constexpr (SEEK) {
      uint32_t lo_i = cur, hi_i = end;
      while (lo_i < hi_i) {
        const uint32_t mid = (lo_i + hi_i) >> 1;
        if (iv[mid].offset + iv[mid].hits <= seg0) lo_i = mid + 1; else hi_i = mid;
      }
      cur = lo_i;
    }
    fold_load_iv(iv, cur, cur < end, off0, hits0);
    fold_load_iv(iv, cur + 1, cur + 1 < end, off1, hits1);
  }
  __device__ __forceinline__ bool empty() const { return cur == end; }

  // does the current interval start before sample c1, the end of the chunk?  (`none` has offset ~0 and ends the walk)
  __device__ __forceinline__ bool before(const uint64_t c1) const { return off0 < c1; }
  // the piece of the current interval inside chunk [c0, c1): samples [s0, s0 + n) of the chunk
  __device__ __forceinline__ void clip(const uint64_t c0, const uint64_t c1, uint32_t& s0, uint32_t& n) const
  {
    const uint64_t lo = off0 > c0 ? off0 : c0;
    const uint64_t hi = off0 + hits0 < c1 ? off0 + hits0 : c1;
    s0 = (uint32_t)(lo - c0);
    n = (uint32_t)(hi - lo);
  }
  // to the next interval; false: the current one continues in the next chunk (or segment)
  template <class IvPtr>
  __device__ __forceinline__ bool advance(const IvPtr iv, const uint64_t c1)
  {
    if (off0 + hits0 > c1) return false;
    cur++;
    off0 = off1;
    hits0 = hits1;
    fold_load_iv(iv, cur + 1, cur + 1 < end, off1, hits1);
    return true;
  }
};

// ---- LONG piece ------------------------------------------------------------------------------------------------------------------
// Samples [s0, s1) of a chunk in the LONG association: singles(h0, h1) adds samples [h0, h1) one by one, blocks(m0, m1) the sums
// of micro-blocks [m0, m1) -- single samples up to the first FOLD_MB boundary inside the piece, whole micro-blocks, single samples
// behind the last boundary; all single samples when no whole micro-block fits.
template <class Singles, class Blocks>
static __device__ __forceinline__ void fold_long_piece(const uint32_t s0, const uint32_t s1, Singles&& singles, Blocks&& blocks)
{
  const uint32_t a0 = (s0 + FOLD_MB - 1) / FOLD_MB * FOLD_MB;                // first micro-block boundary >= s0
  const uint32_t a1 = s1 / FOLD_MB * FOLD_MB;                                // last boundary <= s1
  if (a0 >= a1) {                                                            // no whole micro-block inside the piece
    singles(s0, s1);
  } else {
    singles(s0, a0);
    blocks(a0 / FOLD_MB, a1 / FOLD_MB);
    singles(a1, s1);
  }
}

// ---- run add, dense entry --------------------------------------------------------------------------------------------------------
// acc[r][d] += img[r * RS + h * NDIM + d], h = x0 .. x0 + n - 1 in order: n samples from sample x0 of the chunk image (rows RS
// floats apart), or n micro-block sums.  (h runs over the samples themselves: counted from zero on top of a float offset, the
// register-tight instantiations of k_fold_chunked spill.)
template <uint32_t RS, int NROW, int NDIM>
static __device__ __forceinline__ void fold_run_add(float (&acc)[NROW][NDIM], const float* img, const uint32_t x0, const uint32_t n)
{
#pragma unroll 4
  for (uint32_t h = x0; h < x0 + n; h++)
#pragma unroll
    for (int r = 0; r < NROW; r++)
#pragma unroll
      for (int d = 0; d < NDIM; d++) acc[r][d] += img[r * RS + h * NDIM + d];
}

// entry of the dense table (fold_plan.h plan_dense_fill): first sample of the run inside the chunk | samples << 11; 0: none
static_assert(FOLD_CHUNK == 1u << 11, "dense table entry");
template <uint32_t RS, int NROW, int NDIM>
static __device__ __forceinline__ void fold_dense_add(float (&acc)[NROW][NDIM], const float* img, const uint32_t entry)
{
  fold_run_add<RS>(acc, img, entry & (FOLD_CHUNK - 1), entry >> 11);
}

// ---- accumulators of an owned bin ------------------------------------------------------------------------------------------------
// to floats [x, x + NDIM) of NROW profile rows rs floats apart.  (The load stays a loop in each kernel: as a function that takes
// the accumulators by reference it makes the compiler keep a thread's accumulators as one 16-float vector, and k_fold_dense<4, 1>
// goes from 112 VGPRs to 128 and 188 bytes of scratch; by value, by restrict reference, with the index in 32 or 64 bits alike.)
template <int NROW, int NDIM, class X>
static __device__ __forceinline__ void fold_acc_store(const float (&acc)[NROW][NDIM], float* out, const uint64_t rs, const X x)
{
#pragma unroll
  for (int r = 0; r < NROW; r++)
#pragma unroll
    for (int d = 0; d < NDIM; d++) out[r * rs + (X)(x + d)] = acc[r][d];
}

}  // namespace dspsr_amd
