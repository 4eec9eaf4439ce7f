// Stand-alone driver of dspsr_amd/csrc/fb_inv_walk.h (tests/test_inv_walk_host.py): includes only that header and walks the items of
// every workgroup of one launch of an inverse pass per input line.  Input line:
//   ordered matrix nseg nparts ntile run grid xcd_lr
// Output: one line "ok", or the first property that fails.
//   * every (tile, part) with tile < ntile and part < nparts is dealt exactly once over all workgroups, and nothing else is dealt
//   * a workgroup's sequence ends at the first `false`: the items behind it are `false` as well, as many again as an even share of
//     the launch (ntile * nparts / grid) and eight more
//   * ordered: the items of one (tile, run of parts) all go to one workgroup, parts ascending one by one; run s of a segmented
//     launch holds the parts [s * pps, min(nparts, (s + 1) * pps)), pps = ceil(nparts / nseg), and that is [p0, p0 + np) of the walk
// A workgroup whose run is empty (np == 0) has no item: the kernels leave before they ask for one.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fb_inv_walk.h"

using namespace dspsr_amd;

int main()
{
  long long ordered, matrix, nseg, nparts, ntile, run, grid, lr;
  while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &ordered, &matrix, &nseg, &nparts, &ntile, &run, &grid, &lr) == 8) {
    const char* fail = nullptr;
    const uint32_t NP = (uint32_t)nparts, NT = (uint32_t)ntile, NS = nseg > 1 ? (uint32_t)nseg : 1u;
    std::vector<int> seen((size_t)NT * NP, 0);
    std::vector<int64_t> owner((size_t)NT * NS, -1);          // workgroup of (tile, run of parts)
    const uint32_t pps = (NP + NS - 1) / NS;
    for (uint32_t b = 0; b < (uint32_t)grid && !fail; b++) {
      const InvWalk w = inv_walk(ordered != 0, matrix != 0, (uint32_t)nseg, NP, NT, (uint32_t)run, (uint32_t)grid, b, (int)lr);
      if (ordered) {
        const uint32_t s = NS > 1 ? b / ((uint32_t)grid / NS) : 0u;
        const uint32_t lo = s * pps < NP ? s * pps : NP, hi = (s + 1) * pps < NP ? (s + 1) * pps : NP;
        if (w.seg != s) { fail = "run of the workgroup"; break; }
        if (w.np != hi - lo || (w.np && w.p0 != lo)) { fail = "run s is not the parts [s * pps, min(nparts, (s + 1) * pps))"; break; }
        if (!w.tile_major) { fail = "ordered walk not tile-major"; break; }
        if (w.np == 0) continue;
      }
      InvItem it = {0, 0}, prev = {0, 0};
      uint32_t jj = 0;
      for (; inv_walk_item(w, jj, it); jj++) {
        if (it.tile >= NT || it.lp >= NP) { fail = "item outside the launch"; break; }
        if (seen[(size_t)it.tile * NP + it.lp]++) { fail = "item dealt twice"; break; }
        if (ordered) {
          if (it.lp < w.p0 || it.lp >= w.p0 + w.np) { fail = "part outside the workgroup's run"; break; }
          int64_t& o = owner[(size_t)it.tile * NS + w.seg];
          if (o >= 0 && o != (int64_t)b) { fail = "a (tile, run) goes to two workgroups"; break; }
          o = b;
          const bool first = it.lp == w.p0;
          if (first ? (jj && (prev.lp != w.p0 + w.np - 1 || prev.tile >= it.tile)) : (prev.tile != it.tile || prev.lp + 1 != it.lp)) {
            fail = "parts of a tile not ascending one by one";
            break;
          }
        }
        prev = it;
        if (jj > (uint32_t)NT * NP) { fail = "walk does not end"; break; }
      }
      const uint32_t tail = (uint32_t)((uint64_t)NT * NP / (uint64_t)grid) + 8;
      for (uint32_t k = 1; k <= tail && !fail; k++)
        if (inv_walk_item(w, jj + k, it)) fail = "an item behind the first false";
    }
    for (size_t i = 0; i < seen.size() && !fail; i++)
      if (seen[i] != 1) fail = "an item is dealt to no workgroup";
    printf("%s\n", fail ? fail : "ok");
  }
  return 0;
}
