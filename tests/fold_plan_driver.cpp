// The plan builders of dspsr_amd/csrc/fold_plan.h run stand-alone (tests/test_fold_plan_host.py builds this file with the
// address and undefined-behaviour sanitizers).  Cases are read from stdin until it ends:
//   <op> nbin row_words try_dense first last nkeep npart ndat seg open_hits nrun
//   offset ibin hits                (nrun lines, the runs in time order)
// op: scan | bucket | dense | part | segment.  Every case prints the tables its builder made, one `name: values` line each,
// between `begin` and `end`.  The launch shapes take one line of plain numbers and no runs:
//   fold_shape | many_shape | moments_shape   aligned nchan npol ndim nbin first last max_run dense ncu nslot threads bins_wg
// (threads, bins_wg: k_fold_moments' workgroup) and print `shape: family nd nr grid.x grid.y grid.z threads lds nseg seg_len`.  Every output buffer is a heap block of exactly the size the builder's count function gives, so
// that a write beyond it is an AddressSanitizer report.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>

#include "fold_plan.h"

using namespace dspsr_amd;

static void print_words(const char* name, const uint32_t* p, size_t n)
{
  printf("%s:", name);
  for (size_t i = 0; i < n; i++) printf(" %u", p[i]);
  printf("\n");
}

static void print_iv(const Interval* iv, size_t n)
{
  printf("iv:");
  for (size_t i = 0; i < n; i++) printf(" %" PRIu64 " %u %u", iv[i].offset, iv[i].hits, iv[i].pad);
  printf("\n");
}

int main()
{
  char op[32];
  uint32_t nbin, try_dense, nkeep, npart, seg, open_hits;
  uint64_t row_words, first, last, ndat;
  size_t nrun;
  std::vector<uint32_t> cursor;                    // (the engine's scratch: it lives from case to case, as from call to call)
  while (scanf("%31s", op) == 1) {
    if (!strcmp(op, "fold_shape") || !strcmp(op, "many_shape") || !strcmp(op, "moments_shape")) {
      unsigned aligned, nchan, npol, ndim, max_run, dense, ncu, nslot, mom_threads, mom_bins_wg;
      if (scanf("%u %u %u %u %u %" SCNu64 " %" SCNu64 " %u %u %u %u %u %u", &aligned, &nchan, &npol, &ndim, &nbin, &first, &last, &max_run,
                &dense, &ncu, &nslot, &mom_threads, &mom_bins_wg) != 13) return 2;
      const FoldShape s = !strcmp(op, "fold_shape") ? fold_shape(aligned != 0, nchan, npol, ndim, nbin, first, last, max_run, dense != 0, ncu)
                          : !strcmp(op, "many_shape") ? fold_many_shape(nchan, npol, ndim, nslot, ncu)
                          : fold_moments_shape(nchan, nbin, first, last, max_run, ncu, ndim, mom_threads, mom_bins_wg);
      printf("begin %s\nshape: %d %u %u %u %u %u %u %zu %u %" PRIu64 "\nend\n", op, (int)s.family, s.nd, s.nr, s.grid[0], s.grid[1], s.grid[2],
             s.threads, s.lds, s.nseg, s.seg_len);
      continue;
    }
    if (scanf("%u %" SCNu64 " %u %" SCNu64 " %" SCNu64 " %u %u %" SCNu64 " %u %u %zu", &nbin, &row_words, &try_dense, &first, &last, &nkeep,
              &npart, &ndat, &seg, &open_hits, &nrun) != 11) return 2;
    std::unique_ptr<RunBin[]> runs(new RunBin[nrun]);
    for (size_t i = 0; i < nrun; i++)
      if (scanf("%" SCNu64 " %u %u", &runs[i].offset, &runs[i].ibin, &runs[i].hits) != 3) return 2;
    printf("begin %s\n", op);
    if (!strcmp(op, "scan") || !strcmp(op, "dense")) {
      size_t ntab = 0;
      bool one = false;
      const uint32_t max_run = plan_scan(runs.get(), nrun, nbin, row_words, try_dense != 0, first, last, cursor, &ntab, &one);
      printf("scan: %u %zu %d %u\n", max_run, ntab, one ? 1 : 0, plan_max_run(runs.get(), nrun, open_hits));
      if (!strcmp(op, "dense") && one) {
        std::unique_ptr<uint32_t[]> tab(new uint32_t[ntab]);
        plan_dense_fill(runs.get(), nrun, nbin, first, tab.get(), ntab);
        print_words("tab", tab.get(), ntab);
      }
    } else if (!strcmp(op, "bucket")) {
      std::unique_ptr<uint32_t[]> bin_start(new uint32_t[(size_t)nbin + 1]);
      std::unique_ptr<Interval[]> iv(new Interval[nrun]);
      plan_bucket(runs.get(), nrun, nbin, bin_start.get(), iv.get(), cursor);
      print_words("bin_start", bin_start.get(), (size_t)nbin + 1);
      print_iv(iv.get(), nrun);
    } else if (!strcmp(op, "part")) {
      PartPlanSize sz;
      uint64_t beyond = 0;
      if (!part_plan_count(runs.get(), nrun, nkeep, npart, nbin, cursor, &sz, &beyond)) {
        printf("beyond: %" PRIu64 "\n", beyond);
      } else {
        printf("size: %zu %zu %zu\n", sz.npiece, sz.nentry, sz.nwords);
        std::unique_ptr<uint32_t[]> start(new uint32_t[sz.nwords]);
        std::unique_ptr<Interval[]> iv(new Interval[sz.npiece]);
        part_plan_fill(runs.get(), nrun, nkeep, npart, nbin, cursor, start.get(), iv.get());
        print_words("start", start.get(), sz.nwords);
        print_iv(iv.get(), sz.npiece);
      }
    } else if (!strcmp(op, "segment")) {
      const bool ok = segment_plan_qualifies(runs.get(), nrun, open_hits, ndat, seg);
      printf("qualifies: %d\n", ok ? 1 : 0);
      if (ok) {
        if (open_hits) runs[nrun - 1].hits = open_hits;         // (the engine closes the plan between the two steps)
        const size_t nblk = segment_plan_nblk(ndat);
        std::unique_ptr<uint32_t[]> run_off(new uint32_t[nrun + 1]), blk(new uint32_t[nblk]), bin_start(new uint32_t[(size_t)nbin + 1]);
        std::unique_ptr<Interval[]> iv(new Interval[nrun]);
        segment_plan_fill(runs.get(), nrun, nbin, ndat, run_off.get(), blk.get(), bin_start.get(), iv.get(), cursor);
        print_words("run_off", run_off.get(), nrun + 1);
        print_words("blk_first", blk.get(), nblk);
        print_words("bin_start", bin_start.get(), (size_t)nbin + 1);
        print_iv(iv.get(), nrun);
      }
    } else {
      return 2;
    }
    printf("end\n");
  }
  return feof(stdin) ? 0 : 2;
}
