// Drives HIP::SpectralKurtosisEngine (dspsr_amd/host/dspsr_amd_sk_engine.h) in the reference's call order -- SpectralKurtosis::
// transformation: compute, then detect (reset_mask, detect_tscr, detect_ft, detect_fscr, count_mask / get_estimates / get_zapmask),
// then mask -- against the miniature dsp classes of tests/host_mock, and compares it with the miniature's own CPU engine and with
// the C-ABI driven directly (dspsr_amd_sk_transform).  Rows hold small integers, so every sum is exact and the three must agree
// bit for bit.  Two calls: the counters and the float sums go on.  Built and run by tests/test_sk_adaptor.py.  Exit code 77 = no
// HIP device.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dspsr_amd_engines.h"
#include "dspsr_amd_sk_engine.h"

#define REQUIRE(cond, what) do { if (!(cond)) { printf ("FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); return 1; } } while (0)

static const unsigned NCHAN = 24, NPOL = 2, M = 64, SCHAN = 2, ECHAN = 22;
static const uint64_t NPART = 9, NDAT = NPART * M + 5;

// samples s * t, t in {-1, 0, 1} with P(t != 0) = 1/3 (kurtosis 3: estimates about 1); channel 7 is constant in part 2 (estimate 0:
// an skfb zap), channel 11 twice as strong in the odd parts (a tscr zap), part 5 starts with two strong samples in every channel
static void fill (dsp::TimeSeries& t, unsigned call)
{
  t.set_nchan (NCHAN); t.set_npol (NPOL); t.set_ndim (2); t.set_state (Signal::Analytic); t.set_rate (1e6);
  t.resize (NDAT);
  t.zero ();
  uint32_t s = 12345 + call;
  for (unsigned c = 0; c < NCHAN; c++)
    for (unsigned p = 0; p < NPOL; p++)
      for (uint64_t i = 0; i < 2 * NDAT; i++) {
        s = s * 1664525u + 1013904223u;
        const unsigned r = (s >> 16) % 6;
        float v = r == 0 ? -1.f : r == 1 ? 1.f : 0.f;
        const uint64_t part = (i / 2) / M;
        v *= float (1 + c % 2);
        if (c == 7 && part == 2) v = (i & 1) ? -1.f : 1.f;
        if (c == 11 && (part & 1)) v *= 2.f;
        if (part == 5 && (i / 2) % M < 2) v *= 2.f;
        t.get_datptr (c, p)[i] = v;
      }
}

static void configure (dsp::SpectralKurtosis& sk, const dsp::TimeSeries* in, dsp::TimeSeries* out)
{
  sk.set_input (in);
  sk.set_output (out);
  sk.set_M (M);
  sk.set_thresholds (M, 3);
  sk.set_channel_range (SCHAN, ECHAN);
  sk.set_options (false, false, false);
}

static bool same (const void* a, const void* b, size_t n) { return memcmp (a, b, n) == 0; }

int main ()
{
  try {
    dsp::TimeSeries in_h[2], out_h;
    dsp::SpectralKurtosis sk_h;
    configure (sk_h, &in_h[0], &out_h);
    std::vector<unsigned char> mask_h[2];
    std::vector<float> est_h[2], clean_h[2];
    for (unsigned k = 0; k < 2; k++) {
      fill (in_h[k], k);
      sk_h.set_input (&in_h[k]);
      sk_h.transformation ();
      REQUIRE (sk_h.get_npart () == NPART && out_h.get_ndat () == NPART * M && out_h.get_zeroed_data (), "output of the CPU engine");
      mask_h[k].assign (sk_h.get_mask (), sk_h.get_mask () + NPART * NCHAN);
      est_h[k] = sk_h.get_host_estimates ();
      for (unsigned c = 0; c < NCHAN; c++)
        for (unsigned p = 0; p < NPOL; p++)
          clean_h[k].insert (clean_h[k].end (), out_h.get_datptr (c, p), out_h.get_datptr (c, p) + 2 * NPART * M);
    }
    REQUIRE (sk_h.zap_counts[ZAP_SKFB] && sk_h.zap_counts[ZAP_TSCR] && sk_h.zap_counts[ZAP_FSCR], "every detection must zap something");
    REQUIRE (sk_h.zap_counts[ZAP_ALL] < 2 * NPART * (ECHAN - SCHAN), "something must be kept");
    REQUIRE (sk_h.get_npart_total () == 2 * NPART * NCHAN && sk_h.unfiltered_hits == 2 * NPART, "counters of the CPU engine");
    // without a context the adaptor refuses to come to life
    bool threw = false;
    try { HIP::SpectralKurtosisEngine* bad = new HIP::SpectralKurtosisEngine (0); (void) bad; } catch (Error&) { threw = true; }
    REQUIRE (threw, "HIP::SpectralKurtosisEngine without a context must throw");
    printf ("host engine ok\n");

    dspsr_amd_ctx* ctx = 0;
    if (dspsr_amd_ctx_create (0, DSPSR_AMD_NEW_STREAM, &ctx) != DSPSR_AMD_OK) { printf ("no HIP device\n"); return 77; }
    dsp::Memory* dmem = new HIP::DeviceMemory (ctx);
    dsp::TimeSeries in_d, out_d, out_c;
    in_d.set_memory (dmem); out_d.set_memory (dmem); out_c.set_memory (dmem);
    dsp::SpectralKurtosis sk_d;
    HIP::SpectralKurtosisEngine* eng = new HIP::SpectralKurtosisEngine (ctx, 3);
    eng->set_channel_range (SCHAN, ECHAN);
    configure (sk_d, &in_d, &out_d);
    sk_d.set_engine (eng);
    // the C-ABI driven directly
    dspsr_amd_sk* h = 0;
    REQUIRE (dspsr_amd_sk_create (ctx, &h) == DSPSR_AMD_OK, "create");
    REQUIRE (dspsr_amd_sk_set_shape (h, NCHAN, NPOL, M) == DSPSR_AMD_OK, "set_shape");
    REQUIRE (dspsr_amd_sk_set_options (h, 3, SCHAN, ECHAN, 0, 0, 0) == DSPSR_AMD_OK, "set_options");
    const size_t nrow = 2 * NPART * M;
    std::vector<float> row (nrow), est (NPART * NCHAN * NPOL);
    std::vector<unsigned char> mask (NPART * NCHAN);
    for (unsigned k = 0; k < 2; k++) {
      in_d.internal_match (&in_h[k]);
      REQUIRE (dspsr_amd_copy (ctx, in_d.internal_get_buffer (), in_h[k].internal_get_buffer (), in_h[k].internal_get_size (), DSPSR_AMD_H2D)
               == DSPSR_AMD_OK, "host to device copy");
      sk_d.transformation ();
      REQUIRE (sk_d.get_npart () == NPART && out_d.get_ndat () == NPART * M && out_d.get_zeroed_data (), "output of the adaptor");
      REQUIRE (same (sk_d.get_mask (), &mask_h[k][0], NPART * NCHAN), "adaptor mask differs from the CPU engine's");
      REQUIRE (same (sk_d.get_last_estimates (), &est_h[k][0], est_h[k].size () * sizeof (float)), "adaptor estimates differ from the CPU engine's");
      out_c.copy_configuration (&in_d);
      out_c.resize (NPART * M);
      const float* ib = in_d.get_datptr (0, 0);
      float* ob = out_c.get_datptr (0, 0);
      REQUIRE (dspsr_amd_sk_transform (h, ib, in_d.get_datptr (1, 0) - ib, in_d.get_datptr (0, 1) - ib, ob, out_c.get_datptr (1, 0) - ob,
                                       out_c.get_datptr (0, 1) - ob, NDAT) == DSPSR_AMD_OK, "transform");
      REQUIRE (dspsr_amd_copy (ctx, &est[0], dspsr_amd_sk_estimates_dev (h), est.size () * sizeof (float), DSPSR_AMD_D2H) == DSPSR_AMD_OK, "estimates");
      REQUIRE (dspsr_amd_copy (ctx, &mask[0], dspsr_amd_sk_zapmask_dev (h), mask.size (), DSPSR_AMD_D2H) == DSPSR_AMD_OK, "zapmask");
      REQUIRE (same (&est[0], sk_d.get_last_estimates (), est.size () * sizeof (float)), "C-ABI estimates differ from the adaptor's");
      REQUIRE (same (&mask[0], sk_d.get_mask (), mask.size ()), "C-ABI mask differs from the adaptor's");
      for (unsigned c = 0; c < NCHAN; c++)
        for (unsigned p = 0; p < NPOL; p++) {
          const float* want = &clean_h[k][(size_t (c) * NPOL + p) * nrow];
          REQUIRE (dspsr_amd_copy (ctx, &row[0], out_d.get_datptr (c, p), nrow * sizeof (float), DSPSR_AMD_D2H) == DSPSR_AMD_OK, "copy");
          REQUIRE (same (&row[0], want, nrow * sizeof (float)), "adaptor output differs from the CPU engine's");
          REQUIRE (dspsr_amd_copy (ctx, &row[0], out_c.get_datptr (c, p), nrow * sizeof (float), DSPSR_AMD_D2H) == DSPSR_AMD_OK, "copy");
          REQUIRE (same (&row[0], want, nrow * sizeof (float)), "C-ABI output differs from the CPU engine's");
        }
    }
    // the counters: the CPU engine's against the library's own; the reference's engine branch adds count_mask to ZAP_ALL as well
    uint64_t counts[6];
    std::vector<uint64_t> fhits (NCHAN);
    std::vector<float> fsum (NCHAN * NPOL), usum (NCHAN * NPOL);
    REQUIRE (dspsr_amd_sk_get_statistics (h, counts, &fhits[0], &fsum[0], &usum[0]) == DSPSR_AMD_OK, "get_statistics");
    for (int i = 0; i < 4; i++) REQUIRE (counts[i] == sk_h.zap_counts[i], "zap_counts of the C-ABI");
    REQUIRE (counts[4] == sk_h.get_npart_total () && counts[5] == sk_h.unfiltered_hits, "npart_total / unfiltered_hits of the C-ABI");
    REQUIRE (same (&fhits[0], &sk_h.filtered_hits[0], NCHAN * sizeof (uint64_t)), "filtered_hits of the C-ABI");
    REQUIRE (same (&fsum[0], &sk_h.filtered_sum[0], fsum.size () * sizeof (float)), "filtered_sum of the C-ABI");
    REQUIRE (same (&usum[0], &sk_h.unfiltered_sum[0], usum.size () * sizeof (float)), "unfiltered_sum of the C-ABI");
    REQUIRE (same (&sk_d.filtered_sum[0], &sk_h.filtered_sum[0], fsum.size () * sizeof (float)), "filtered_sum through the adaptor");
    REQUIRE (same (&sk_d.filtered_hits[0], &sk_h.filtered_hits[0], NCHAN * sizeof (uint64_t)), "filtered_hits through the adaptor");
    for (int i = 1; i < 4; i++) REQUIRE (sk_d.zap_counts[i] == 0, "the engine branch of the reference keeps no per-detection counts");
    unsigned all = 0;
    for (unsigned k = 0; k < 2; k++) for (size_t i = 0; i < mask_h[k].size (); i++) all += mask_h[k][i];
    REQUIRE (sk_d.zap_counts[ZAP_ALL] == sk_h.zap_counts[ZAP_ALL] + all, "ZAP_ALL through the adaptor: count_mask plus the host loop");
    dspsr_amd_sk_destroy (h);
    printf ("sk adaptor driver ok\n");
    return 0;
  } catch (Error& e) {
    printf ("FAILED: Error %s\n", e.message.c_str ());
    return 1;
  }
}
