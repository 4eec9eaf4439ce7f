// FUNCTIONAL MINIATURE (see ../Error.h): dsp::SpectralKurtosis and its Engine interface (Signal/General/dsp/SpectralKurtosis.h:
// 24-214), reduced to what the adaptor dspsr_amd/host/dspsr_amd_sk_engine.h touches.  transformation() makes the engine calls in
// the order of Signal/General/SpectralKurtosis.C:194-232,413-454,605-665,747-797; without an engine it runs a small CPU engine of
// the FPT branch.  The zap mask is a BitSeries of one byte per (part, channel); the limits come from dspsr_amd_sk_limits, the
// product's port of dsp::SKLimits.
#pragma once
#include <math.h>

#include "dsp/Memory.h"
#include "dspsr_amd.h"

#define ZAP_ALL  0
#define ZAP_SKFB 1
#define ZAP_FSCR 2
#define ZAP_TSCR 3

namespace dsp {
  class SpectralKurtosis : public Reference::Able {
  public:
    class Engine;
    SpectralKurtosis () : input (0), output (0), M (128), nchan (0), npol (0), npart (0), unfiltered_hits (0), std_devs (3),
                          npart_total (0)
    {
      estimates = new TimeSeries; estimates_tscr = new TimeSeries; zapmask = new BitSeries;
      thresholds[0] = thresholds[1] = 0;
      channels[0] = channels[1] = 0;
      detection_flags[0] = detection_flags[1] = detection_flags[2] = false;
      for (int i = 0; i < 4; i++) zap_counts[i] = 0;
    }
    void set_input (const TimeSeries* in) { input = in; }
    void set_output (TimeSeries* out) { output = out; }
    void set_M (unsigned _M) { M = _M; }
    void set_thresholds (unsigned _M, unsigned _std_devs)                       // SpectralKurtosis.C:380-397
    {
      M = _M; std_devs = _std_devs;
      if (dspsr_amd_sk_limits (M, std_devs, &thresholds[0], &thresholds[1]) != DSPSR_AMD_OK)
        throw Error (InvalidParam, "dsp::SpectralKurtosis::set_thresholds", "SKLimits invalid inputs M=%u std_devs=%u", M, std_devs);
    }
    void set_channel_range (unsigned start, unsigned end) { channels[0] = start; channels[1] = end; }
    void set_options (bool no_fscr, bool no_tscr, bool no_ft)
    { detection_flags[0] = no_fscr; detection_flags[1] = no_tscr; detection_flags[2] = no_ft; }
    void set_engine (Engine* e) { engine = e; }
    void reset_count () { unfiltered_hits = 0; }

    inline void transformation ();                                              // :194-232

    // what the tests read
    uint64_t get_npart () const { return npart; }
    const std::vector<float>& get_host_estimates () const { return est; }       // CPU branch only
    const std::vector<float>& get_host_estimates_tscr () const { return est_tscr; }
    const unsigned char* get_mask () const { return last_mask; }                // [npart][nchan] of the last call
    const float* get_last_estimates () const { return last_estimates; }
    uint64_t zap_counts[4], unfiltered_hits;
    std::vector<float> filtered_sum, unfiltered_sum;
    std::vector<uint64_t> filtered_hits;
    uint64_t get_npart_total () const { return npart_total; }

  protected:
    inline void compute ();
    inline void detect ();
    inline void detect_tscr ();
    inline void detect_skfb ();
    inline void detect_fscr ();
    inline void count_zapped ();
    inline void mask ();
    inline void reset_mask ();

    const TimeSeries* input;
    TimeSeries* output;
    Reference::To<Engine> engine;
    Reference::To<TimeSeries> estimates, estimates_tscr;
    Reference::To<BitSeries> zapmask;
    unsigned M, nchan, npol;
    uint64_t npart;
    unsigned std_devs;
    float thresholds[2];
    unsigned channels[2];
    bool detection_flags[3];                                                    // [0:fscr, 1:tscr, 2:ft]
    uint64_t npart_total;
    std::vector<uint64_t> thresholds_tscr_m;
    std::vector<float> thresholds_tscr_lower, thresholds_tscr_upper;
    std::vector<float> est, est_tscr, S1_tscr, S2_tscr;                          // the CPU branch's estimates (TFP) and sums
    const unsigned char* last_mask;
    const float* last_estimates;
  };

  class SpectralKurtosis::Engine : public Reference::Able {                      // SpectralKurtosis.h:181-214
  public:
    virtual void setup () = 0;
    virtual void compute (const TimeSeries* input, TimeSeries* output, TimeSeries* output_tscr, unsigned tscrunch) = 0;
    virtual void reset_mask (BitSeries* output) = 0;
    virtual void detect_ft (const TimeSeries* input, BitSeries* output, float upper_thresh, float lower_thresh) = 0;
    virtual void detect_fscr (const TimeSeries* input, BitSeries* output, const float lower, const float upper, unsigned schan,
                              unsigned echan) = 0;
    virtual void detect_tscr (const TimeSeries* input, const TimeSeries* input_tscr, BitSeries* output, float upper, float lower) = 0;
    virtual int count_mask (const BitSeries* output) = 0;
    virtual float* get_estimates (const TimeSeries* input) = 0;
    virtual unsigned char* get_zapmask (const BitSeries* input) = 0;
    virtual void mask (BitSeries* mask, const TimeSeries* in, TimeSeries* out, unsigned M) = 0;
    virtual void insertsk (const TimeSeries* input, TimeSeries* out, unsigned M) = 0;
  };

  void SpectralKurtosis::transformation ()
  {
    nchan = input->get_nchan (); npol = input->get_npol ();
    if (input->get_ndim () != 2)
      throw Error (InvalidState, "dsp::SpectralKurtosis::transformation", "only complex (ndim 2) input");
    const uint64_t ndat = input->get_ndat ();
    npart = ndat / M;                                                           // :204
    output->copy_configuration (input);                                         // prepare_output
    estimates->set_nchan (nchan); estimates->set_npol (npol); estimates->set_ndim (1);     // reserve, :170-191
    estimates->resize (npart);
    estimates_tscr->set_nchan (nchan); estimates_tscr->set_npol (npol); estimates_tscr->set_ndim (1);
    estimates_tscr->resize (npart > 0);
    zapmask->set_nchan (nchan);
    zapmask->resize (npart, nchan);
    output->resize (npart * M);
    if (ndat == 0 || npart == 0) return;
    compute ();
    detect ();
    mask ();
  }

  void SpectralKurtosis::compute ()                                             // :234-372, FPT order
  {
    if (engine) { engine->compute (input, estimates, estimates_tscr, M); return; }
    S1_tscr.assign (nchan * npol, 0.f); S2_tscr.assign (nchan * npol, 0.f);
    est.assign (npart * nchan * npol, 0.f);
    const float M_fac = (M + 1) / (M - 1);                                      // unsigned integer division
    for (uint64_t ipart = 0; ipart < npart; ipart++)
      for (unsigned ichan = 0; ichan < nchan; ichan++)
        for (unsigned ipol = 0; ipol < npol; ipol++) {
          const float* p = input->get_datptr (ichan, ipol) + ipart * 2 * M;
          float S1 = 0, S2 = 0;
          for (unsigned i = 0; i < 2 * M; i += 2) {
            const float sqld = (p[i] * p[i]) + (p[i + 1] * p[i + 1]);
            S1 += sqld;
            S2 += (sqld * sqld);
          }
          if (!detection_flags[1]) { S1_tscr[ichan * npol + ipol] += S1; S2_tscr[ichan * npol + ipol] += S2; }
          est[(ipart * nchan + ichan) * npol + ipol] = S1 == 0 ? 0 : M_fac * (M * (S2 / (S1 * S1)) - 1);
        }
    if (!detection_flags[1]) {
      est_tscr.assign (nchan * npol, 0.f);
      const float M_t = (float) (M * npart);
      const float M_fac_t = (M_t + 1) / (M_t - 1);
      for (unsigned i = 0; i < nchan * npol; i++)
        est_tscr[i] = S1_tscr[i] == 0 ? 0 : M_fac_t * (M_t * (S2_tscr[i] / (S1_tscr[i] * S1_tscr[i])) - 1);
    }
  }

  void SpectralKurtosis::detect ()                                              // :413-454
  {
    if (channels[1] == 0) channels[1] = nchan;
    npart_total += npart * nchan;
    reset_mask ();
    if (!detection_flags[1]) detect_tscr ();
    if (!detection_flags[2]) detect_skfb ();
    if (!detection_flags[0]) detect_fscr ();
    count_zapped ();
  }

  void SpectralKurtosis::reset_mask ()
  {
    if (engine) { engine->reset_mask (zapmask); return; }
    memset (zapmask->get_rawptr (), 0, npart * nchan);
  }

  void SpectralKurtosis::detect_tscr ()                                         // :459-538
  {
    const uint64_t m = uint64_t (M) * npart;
    float lower = 0, upper = 0;
    bool must_compute = true;
    for (unsigned i = 0; i < thresholds_tscr_m.size (); i++)
      if (thresholds_tscr_m[i] == m) { must_compute = false; lower = thresholds_tscr_lower[i]; upper = thresholds_tscr_upper[i]; }
    if (must_compute) {
      const unsigned M_tscr = (unsigned) float (m);
      if (dspsr_amd_sk_limits (M_tscr, std_devs, &lower, &upper) != DSPSR_AMD_OK)
        throw Error (InvalidParam, "dsp::SpectralKurtosis::detect_tscr", "SKLimits invalid inputs");
      thresholds_tscr_m.push_back (m); thresholds_tscr_lower.push_back (lower); thresholds_tscr_upper.push_back (upper);
    }
    if (engine) { engine->detect_tscr (estimates, estimates_tscr, zapmask, upper, lower); return; }
    unsigned char* out = zapmask->get_rawptr ();
    for (unsigned ichan = channels[0]; ichan < channels[1]; ichan++) {
      bool zap = false;
      for (unsigned ipol = 0; ipol < npol; ipol++) {
        const float V = est_tscr[ichan * npol + ipol];
        if (V > upper || V < lower) zap = true;
      }
      if (zap)
        for (uint64_t ipart = 0; ipart < npart; ipart++) { out[ipart * nchan + ichan] = 1; zap_counts[ZAP_TSCR]++; }
    }
  }

  void SpectralKurtosis::detect_skfb ()                                         // :540-584
  {
    if (engine) { engine->detect_ft (estimates, zapmask, thresholds[1], thresholds[0]); return; }
    unsigned char* out = zapmask->get_rawptr ();
    for (uint64_t ipart = 0; ipart < npart; ipart++)
      for (unsigned ichan = 0; ichan < nchan; ichan++) {
        bool zap = false;
        for (unsigned ipol = 0; ipol < npol; ipol++) {
          const float V = est[(ipart * nchan + ichan) * npol + ipol];
          if (V > thresholds[1] || V < thresholds[0]) zap = true;
        }
        if (zap) {
          out[ipart * nchan + ichan] = 1;
          if (ichan > channels[0] && ichan < channels[1]) zap_counts[ZAP_SKFB]++;
        }
      }
  }

  void SpectralKurtosis::detect_fscr ()                                         // :667-743
  {
    const float _M = (float) M;
    const float mu2 = (4 * _M * _M) / ((_M - 1) * (_M + 2) * (_M + 3));
    if (engine) {
      const float one_sigma_idat = sqrtf (mu2 / (float) nchan);
      const float upper = 1 + ((1 + std_devs) * one_sigma_idat), lower = 1 - ((1 + std_devs) * one_sigma_idat);
      engine->detect_fscr (estimates, zapmask, lower, upper, channels[0], channels[1]);
      return;
    }
    unsigned char* out = zapmask->get_rawptr ();
    for (uint64_t ipart = 0; ipart < npart; ipart++) {
      bool zap_ipart = false;
      for (unsigned ipol = 0; ipol < npol; ipol++) {
        float sk_avg = 0;
        unsigned cnt = 0;
        for (unsigned ichan = channels[0]; ichan < channels[1]; ichan++)
          if (out[ipart * nchan + ichan] == 0) { sk_avg += est[(ipart * nchan + ichan) * npol + ipol]; cnt++; }
        if (cnt > 0) {
          sk_avg /= (float) cnt;
          const float one_sigma_idat = sqrtf (mu2 / (float) cnt);
          const float up = 1 + ((1 + std_devs) * one_sigma_idat), lo = 1 - ((1 + std_devs) * one_sigma_idat);
          if (sk_avg > up || sk_avg < lo) zap_ipart = true;
        }
      }
      if (zap_ipart) {
        for (unsigned ichan = 0; ichan < nchan; ichan++) out[ipart * nchan + ichan] = 1;
        zap_counts[ZAP_FSCR] += nchan;
      }
    }
  }

  void SpectralKurtosis::count_zapped ()                                        // :605-665
  {
    const float* indat;
    const unsigned char* outdat;
    if (engine) {
      const int zapped = engine->count_mask (zapmask);
      indat = engine->get_estimates (estimates);
      outdat = engine->get_zapmask (zapmask);
      zap_counts[ZAP_ALL] += zapped;
    } else {
      indat = &est[0];
      outdat = zapmask->get_rawptr ();
    }
    last_mask = outdat; last_estimates = indat;
    if (unfiltered_hits == 0) {
      filtered_sum.assign (npol * nchan, 0.f); unfiltered_sum.assign (npol * nchan, 0.f); filtered_hits.assign (nchan, 0);
    }
    for (uint64_t ipart = 0; ipart < npart; ipart++) {
      unfiltered_hits++;
      for (unsigned ichan = channels[0]; ichan < channels[1]; ichan++) {
        const uint64_t index = (ipart * nchan + ichan) * npol;
        const unsigned outdex = ichan * npol;
        for (unsigned ipol = 0; ipol < npol; ipol++) unfiltered_sum[outdex + ipol] += indat[index + ipol];
        if (outdat[ipart * nchan + ichan] == 1) { zap_counts[ZAP_ALL]++; continue; }
        for (unsigned ipol = 0; ipol < npol; ipol++) filtered_sum[outdex + ipol] += indat[index + ipol];
        filtered_hits[ichan]++;
      }
    }
  }

  void SpectralKurtosis::mask ()                                                // :747-801
  {
    output->set_zeroed_data (true);
    if (engine) { engine->mask (zapmask, input, output, M); return; }
    const unsigned char* m = zapmask->get_rawptr ();
    for (unsigned ichan = 0; ichan < nchan; ichan++)
      for (unsigned ipol = 0; ipol < npol; ipol++) {
        const float* in = input->get_datptr (ichan, ipol);
        float* out = output->get_datptr (ichan, ipol);
        for (uint64_t ipart = 0; ipart < npart; ipart++)
          for (unsigned j = 0; j < 2 * M; j++)
            out[ipart * 2 * M + j] = m[ipart * nchan + ichan] ? 0.f : in[ipart * 2 * M + j];
      }
  }
}
