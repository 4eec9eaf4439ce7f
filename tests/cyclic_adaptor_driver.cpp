// Drives HIP::CyclicFoldEngine (dspsr_amd/host/dspsr_amd_cyclic_engine.h) in the reference's call order -- CyclicFold::prepare
// (set_nlag, set_mover, set_npol, set_profiles), prepare_output, then per Fold::fold: set_nbin, set_ndat, set_bin x ndat, fold;
// get_result -> synch; reset -> zero -- against the miniature dsp classes of tests/host_mock, and compares it with the
// miniature's own CPU engine and with the C-ABI driven directly.  Rows hold integers in [-7, 7], so every sum is exact and the
// three must agree bit for bit.  Built and run by tests/test_cyclic_adaptor.py.  Exit code 77 = no HIP device.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dspsr_amd_engines.h"
#include "dspsr_amd_cyclic_engine.h"

#define REQUIRE(cond, what) do { if (!(cond)) { printf ("FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); return 1; } } while (0)

struct HostEngine : public dsp::CyclicFoldEngine {
  const float* lags () const { return lagdata; }
  uint64_t nlags () const { return lagdata_size; }
};

static const unsigned NCHAN = 2, NPOL = 2, NBIN = 8, NCYC = 32;
static const uint64_t NDAT = 700;
struct Call { double phi, pfold; uint64_t start, ndat; };
static const Call CALLS[2] = { { 0.3, 8 * 9.3e-6, 0, 400 }, { -2.6, 8 * 0.7e-6, 400, 300 } };

static void fill (dsp::TimeSeries& t)
{
  t.set_nchan (NCHAN); t.set_npol (NPOL); t.set_ndim (2); t.set_state (Signal::Analytic); t.set_rate (1e6);
  t.resize (NDAT);
  t.zero ();
  uint32_t s = 12345;
  for (unsigned c = 0; c < NCHAN; c++)
    for (unsigned p = 0; p < NPOL; p++)
      for (uint64_t i = 0; i < 2 * NDAT; i++) {
        s = s * 1664525u + 1013904223u;
        t.get_datptr (c, p)[i] = float (int ((s >> 16) % 15) - 7);
      }
}

static void run (dsp::CyclicFold& cf, const dsp::TimeSeries* in, dsp::Fold::Engine* engine, unsigned mover, unsigned npol_out)
{
  cf.set_input (in);
  cf.set_nbin (NBIN);
  cf.set_mover (mover);
  cf.set_nchan (NCYC);
  cf.set_npol (npol_out);
  cf.set_engine (engine);
  cf.prepare ();
  for (int k = 0; k < 2; k++) {
    cf.prepare_output ();
    cf.fold (CALLS[k].phi, CALLS[k].pfold, CALLS[k].start, CALLS[k].ndat);
  }
}

static bool same (const float* a, const float* b, uint64_t n) { return memcmp (a, b, n * sizeof (float)) == 0; }

int main ()
{
  try {
    dsp::TimeSeries in_h;
    fill (in_h);
    // the miniature's CPU engine on its own: the call order works without a device
    {
      dsp::CyclicFold cf;
      HostEngine* e = new HostEngine;
      run (cf, &in_h, e, 1, 4);
      const unsigned nlag = NCYC / 2 + 1, n = NCYC;
      std::vector<float> spectra (uint64_t (NCHAN) * n * 4 * NBIN);
      REQUIRE (dspsr_amd_cyclic_lags_to_spectra (e->lags (), NCHAN, 4, NBIN, nlag, 1, &spectra[0]) == DSPSR_AMD_OK, "lags_to_spectra");
      dsp::PhaseSeries* r = cf.get_result ();
      // the library's float radix-2 transform against the miniature's double sum: (log2 n + 1) * 2^-23 of the largest value
      // of the auto spectra (the cross products are bounded by them)
      double worst = 0, peak = 0;
      for (unsigned c = 0; c < NCHAN * n; c++)
        for (unsigned p = 0; p < 4; p++)
          for (unsigned b = 0; b < NBIN; b++) {
            const double want = r->get_datptr (c, p)[b], got = spectra[(uint64_t (c) * 4 + p) * NBIN + b];
            if (fabs (got - want) > worst) worst = fabs (got - want);
            if (p < 2 && fabs (want) > peak) peak = fabs (want);
          }
      printf ("lags_to_spectra against the base synch: %.3g of the peak\n", worst / peak);
      REQUIRE (worst <= (log2 (double (n)) + 1) * ldexp (1.0, -23) * peak, "lags_to_spectra differs from the base synch");
      REQUIRE (r->get_nchan () == NCHAN * NCYC && r->get_npol () == 4 && r->get_ndim () == 1 && r->get_nbin () == NBIN, "output shape");
      REQUIRE (e->nlags () == uint64_t (NCYC / 2 + 1) * NBIN * 4 * 2 * NCHAN, "lag data size");
    }
    // without a context the adaptor refuses to come to life
    bool threw = false;
    try { HIP::CyclicFoldEngine* bad = new HIP::CyclicFoldEngine (0); (void) bad; } catch (Error&) { threw = true; }
    REQUIRE (threw, "HIP::CyclicFoldEngine without a context must throw");
    printf ("host engine ok\n");

    dspsr_amd_ctx* ctx = 0;
    if (dspsr_amd_ctx_create (0, DSPSR_AMD_NEW_STREAM, &ctx) != DSPSR_AMD_OK) { printf ("no HIP device\n"); return 77; }
    dsp::Memory* dmem = new HIP::DeviceMemory (ctx);
    dsp::TimeSeries in_d;
    in_d.set_memory (dmem);
    in_d.internal_match (&in_h);
    REQUIRE (in_d.internal_get_size () == in_h.internal_get_size (), "device copy of the input");
    REQUIRE (dspsr_amd_copy (ctx, in_d.internal_get_buffer (), in_h.internal_get_buffer (), in_h.internal_get_size (), DSPSR_AMD_H2D)
             == DSPSR_AMD_OK, "host to device copy");

    for (unsigned mover = 1; mover <= 2; mover++) {
      const unsigned npol_out = mover == 1 ? 4 : 2, nlag = mover * NCYC / 2 + 1;
      dsp::CyclicFold cf_h, cf_d;
      HostEngine* he = new HostEngine;
      HIP::CyclicFoldEngine* de = new HIP::CyclicFoldEngine (ctx);
      run (cf_h, &in_h, he, mover, npol_out);
      run (cf_d, &in_d, de, mover, npol_out);
      const uint64_t nl = he->nlags ();
      REQUIRE (de->get_lagdata_size () == nl, "lag data sizes");
      // the C-ABI driven directly, the same plan through set_bin
      dspsr_amd_cyclic_fold* h = 0;
      REQUIRE (dspsr_amd_cyclic_fold_create (ctx, &h) == DSPSR_AMD_OK, "create");
      REQUIRE (dspsr_amd_cyclic_fold_set_shape (h, NCHAN, NPOL, npol_out, nlag, mover, NBIN) == DSPSR_AMD_OK, "set_shape");
      for (int k = 0; k < 2; k++) {
        double phi = CALLS[k].phi;
        const double pps = 1e-6 / CALLS[k].pfold;
        REQUIRE (dspsr_amd_cyclic_fold_set_ndat (h, CALLS[k].ndat, CALLS[k].start) == DSPSR_AMD_OK, "set_ndat");
        for (uint64_t i = CALLS[k].start; i < CALLS[k].start + CALLS[k].ndat; i++) {
          phi -= floor (phi);
          REQUIRE (dspsr_amd_cyclic_fold_set_bin (h, i, phi * NBIN, pps * NBIN) == DSPSR_AMD_OK, "set_bin");
          phi += pps;
        }
        REQUIRE (dspsr_amd_cyclic_fold_fold (h, in_d.get_datptr (0, 0), in_d.get_datptr (1, 0) - in_d.get_datptr (0, 0),
                                             in_d.get_datptr (0, 1) - in_d.get_datptr (0, 0)) == DSPSR_AMD_OK, "fold");
      }
      std::vector<float> direct (nl);
      REQUIRE (dspsr_amd_cyclic_fold_synch_lags (h, &direct[0]) == DSPSR_AMD_OK, "synch_lags");
      std::vector<float> host_lags (he->lags (), he->lags () + nl);       // before synch windows them in place
      REQUIRE (same (&host_lags[0], &direct[0], nl), "C-ABI lag data differ from the CPU engine's");
      bool any = false;
      for (uint64_t i = 0; i < nl; i++) any = any || direct[i] != 0.f;
      REQUIRE (any, "lag data are all zero");
      dsp::PhaseSeries* rh = cf_h.get_result ();                          // Fold::get_result -> engine->synch
      dsp::PhaseSeries* rd = cf_d.get_result ();
      if (mover == 1)                                                      // no window: the adaptor's host copy is the device's
        REQUIRE (same (de->get_lagdata (), &direct[0], nl), "adaptor lag data differ from the C-ABI path");
      REQUIRE (same (de->get_lagdata (), he->lags (), nl), "adaptor lag data differ from the CPU engine's (after synch)");
      const unsigned nout = NCHAN * (2 * nlag - 2) / mover;
      REQUIRE (rd->get_nchan () == nout && rd->get_npol () == npol_out && rd->get_nbin () == NBIN, "adaptor output shape");
      for (unsigned c = 0; c < nout; c++)
        for (unsigned p = 0; p < npol_out; p++)
          REQUIRE (same (rd->get_datptr (c, p), rh->get_datptr (c, p), NBIN), "adaptor spectra differ from the CPU engine's");
      for (unsigned b = 0; b < NBIN; b++) REQUIRE (rd->get_hits ()[b] == rh->get_hits ()[b], "hits");
      REQUIRE (rd->ndat_total == NDAT, "ndat_total");
      cf_d.reset ();                                                       // Engine::zero
      REQUIRE (dspsr_amd_cyclic_fold_synch_lags (h, &direct[0]) == DSPSR_AMD_OK, "synch_lags");
      dspsr_amd_cyclic_fold_destroy (h);
      for (uint64_t i = 0; i < nl; i++) REQUIRE (de->get_lagdata ()[i] == 0.f, "zero() must clear the host lag data");
    }
    printf ("cyclic adaptor driver ok\n");
    return 0;
  } catch (Error& e) {
    printf ("FAILED: Error %s\n", e.message.c_str ());
    return 1;
  }
}
