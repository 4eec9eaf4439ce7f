// Stand-alone driver for the host code of dspsr -R (csrc/host_prep.cpp: dspsr_amd_rfi_mask_calculate, dspsr_amd_rfi_mask_expand,
// dspsr_amd_response_multiply): tests/test_rfi_host.py builds it together with host_prep.cpp under the address and undefined-behaviour
// sanitizers and runs its cases through it.  Records of `in`:  u32 op, then
//   1 calculate: u32 n, window, keep; float p0[n], p1[n]        -> i32 rc; u32 total, rounds; float mask[n], p0[n], p1[n], cutoffs[n + 2]
//   2 expand   : u32 n; u64 required; float mask[n]             -> i32 rc; float phasors[2 required]
//   3 multiply : u64 ncomplex; float kernel[2 n], phasors[2 n]  -> i32 rc; float kernel[2 n]
// Every array is an exactly sized heap block, so that one element past its end is a sanitizer error.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "dspsr_amd.h"

template <typename T> static bool get(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T> static void put(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint32_t op;
  while (get(in, &op, 1)) {
    if (op == 1) {
      uint32_t h[3];
      if (!get(in, h, 3)) return 3;
      const uint32_t n = h[0];
      std::vector<float> p0(n), p1(n), mask(n), cut(n + 2, 0.f);
      if (!get(in, p0.data(), n) || !get(in, p1.data(), n)) return 3;
      uint32_t tr[2] = {0, 0};
      const int32_t rc = dspsr_amd_rfi_mask_calculate_log(p0.data(), p1.data(), n, h[1], (int)h[2], mask.data(), &tr[0], &tr[1],
                                                          cut.data(), n + 2);
      // the entry point without the log gives the same mask and counts
      std::vector<float> q0(n), q1(n), m2(n);
      fseek(in, -(long)(2 * n * sizeof(float)), SEEK_CUR);
      if (!get(in, q0.data(), n) || !get(in, q1.data(), n)) return 3;
      uint32_t tr2[2] = {0, 0};
      const int32_t rc2 = dspsr_amd_rfi_mask_calculate(q0.data(), q1.data(), n, h[1], (int)h[2], m2.data(), &tr2[0], &tr2[1]);
      if (rc2 != rc || tr2[0] != tr[0] || tr2[1] != tr[1] || m2 != mask || q0 != p0 || q1 != p1) return 4;
      put(out, &rc, 1);
      put(out, tr, 2);
      put(out, mask.data(), n);
      put(out, p0.data(), n);
      put(out, p1.data(), n);
      put(out, cut.data(), n + 2);
    } else if (op == 2) {
      uint32_t n;
      uint64_t required;
      if (!get(in, &n, 1) || !get(in, &required, 1)) return 3;
      std::vector<float> mask(n), ph(2 * required);
      if (!get(in, mask.data(), n)) return 3;
      const int32_t rc = dspsr_amd_rfi_mask_expand(mask.data(), n, required, ph.data());
      put(out, &rc, 1);
      put(out, ph.data(), ph.size());
    } else if (op == 3) {
      uint64_t n;
      if (!get(in, &n, 1)) return 3;
      std::vector<float> k(2 * n), ph(2 * n);
      if (!get(in, k.data(), 2 * n) || !get(in, ph.data(), 2 * n)) return 3;
      const int32_t rc = dspsr_amd_response_multiply(k.data(), ph.data(), n);
      put(out, &rc, 1);
      put(out, k.data(), k.size());
    } else {
      return 5;
    }
  }
  fclose(out);
  return 0;
}
