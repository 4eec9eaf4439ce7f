// dspsr_amd_sk_engine.h -- HIP::SpectralKurtosisEngine: dsp::SpectralKurtosis::Engine (Signal/General/dsp/SpectralKurtosis.h:
// 181-214) over the C-ABI of include/dspsr_amd.h (dspsr_amd_sk_*), in the place of CUDA::SpectralKurtosisEngine.
//
// The estimates and the zap mask live in the library's object on the device.  dsp::SpectralKurtosis never reads the containers it
// hands to its engine (estimates, estimates_tscr, zapmask: it sizes them and passes them through); what it reads on the host, in
// count_zapped, it asks of get_estimates / get_zapmask, which copy into host buffers this class owns.  The input and output
// TimeSeries live on the device (HIP::DeviceMemory).  The detection is the CPU branch's (SpectralKurtosis.C:459-743), which is
// the definition: detect_fscr ignores the limits of the engine branch (:677-680, computed for all nchan channels) and applies
// the per-part limits of :711-726 to the channels of [schan, echan) not yet zapped.
// detect_tscr and detect_ft receive no channel range from their caller: they use the range of the last detect_fscr, or the one
// given to set_channel_range (call it where skestimator->set_channel_range is called, LoadToFold1.C:527-528); all channels
// otherwise.  Installed where the CUDA engine is (LoadToFold1.C:516-524):
//   skestimator->set_engine (new HIP::SpectralKurtosisEngine (ctx, config->sk_std_devs));
#ifndef DSPSR_AMD_SK_ENGINE_H
#define DSPSR_AMD_SK_ENGINE_H

#include <vector>

#include "dsp/SpectralKurtosis.h"

#include "dspsr_amd_adaptor_common.h"   // HIP::check, HIP::rows_of

namespace HIP
{
  class SpectralKurtosisEngine : public dsp::SpectralKurtosis::Engine
  {
  public:
    SpectralKurtosisEngine (dspsr_amd_ctx* _ctx, unsigned _std_devs = 3)
      : ctx (_ctx), handle (0), std_devs (_std_devs), chan_start (0), chan_end (0), nchan (0), npol (0)
    { status (dspsr_amd_sk_create (ctx, &handle), "HIP::SpectralKurtosisEngine"); }
    ~SpectralKurtosisEngine () { if (handle) dspsr_amd_sk_destroy (handle); }

    void setup () { }

    //! the range SpectralKurtosis::set_channel_range was given; end 0: all channels from start
    void set_channel_range (unsigned start, unsigned end) { chan_start = start; chan_end = end; }

    void compute (const dsp::TimeSeries* input, dsp::TimeSeries*, dsp::TimeSeries*, unsigned tscrunch)
    {
      if (input->get_memory ()->on_host ())
        throw Error (InvalidState, "HIP::SpectralKurtosisEngine::compute", "the input TimeSeries is not in device memory");
      if (input->get_ndim () != 2)
        throw Error (InvalidState, "HIP::SpectralKurtosisEngine::compute", "only complex (ndim 2) input");
      nchan = input->get_nchan (); npol = input->get_npol ();
      status (dspsr_amd_sk_set_shape (handle, nchan, npol, tscrunch), "HIP::SpectralKurtosisEngine::compute");
      options ("HIP::SpectralKurtosisEngine::compute");
      const Rows<const float*> rows = rows_of (input);
      status (dspsr_amd_sk_compute (handle, rows.base, rows.cs, rows.ps, input->get_ndat ()), "HIP::SpectralKurtosisEngine::compute");
    }

    void reset_mask (dsp::BitSeries*) { status (dspsr_amd_sk_reset_mask (handle), "HIP::SpectralKurtosisEngine::reset_mask"); }

    void detect_ft (const dsp::TimeSeries*, dsp::BitSeries*, float upper_thresh, float lower_thresh)
    { status (dspsr_amd_sk_detect_skfb (handle, lower_thresh, upper_thresh), "HIP::SpectralKurtosisEngine::detect_ft"); }

    void detect_fscr (const dsp::TimeSeries*, dsp::BitSeries*, const float, const float, unsigned schan, unsigned echan)
    {
      chan_start = schan; chan_end = echan;
      options ("HIP::SpectralKurtosisEngine::detect_fscr");
      status (dspsr_amd_sk_detect_fscr (handle), "HIP::SpectralKurtosisEngine::detect_fscr");
    }

    void detect_tscr (const dsp::TimeSeries*, const dsp::TimeSeries*, dsp::BitSeries*, float upper, float lower)
    { status (dspsr_amd_sk_detect_tscr (handle, lower, upper), "HIP::SpectralKurtosisEngine::detect_tscr"); }

    //! the number of zapped (part, channel) pairs of the mask
    int count_mask (const dsp::BitSeries*)
    {
      fetch_mask ("HIP::SpectralKurtosisEngine::count_mask");
      int n = 0;
      for (size_t i = 0; i + 1 < host_mask.size (); i++) n += host_mask[i] != 0;
      return n;
    }

    float* get_estimates (const dsp::TimeSeries*)
    {
      host_estimates.resize (size_t (dspsr_amd_sk_npart (handle)) * nchan * npol + 1);
      status (dspsr_amd_copy (ctx, &host_estimates[0], dspsr_amd_sk_estimates_dev (handle), (host_estimates.size () - 1) * sizeof (float),
                              DSPSR_AMD_D2H), "HIP::SpectralKurtosisEngine::get_estimates");
      return &host_estimates[0];
    }

    unsigned char* get_zapmask (const dsp::BitSeries*)
    {
      fetch_mask ("HIP::SpectralKurtosisEngine::get_zapmask");
      return &host_mask[0];
    }

    void mask (dsp::BitSeries*, const dsp::TimeSeries* in, dsp::TimeSeries* out, unsigned)
    {
      if (in->get_memory ()->on_host () || out->get_memory ()->on_host ())
        throw Error (InvalidState, "HIP::SpectralKurtosisEngine::mask", "the TimeSeries are not in device memory");
      // the shape remembered from compute (), the one the library object holds, for both series
      const Rows<const float*> i = rows_of (in, nchan, npol);
      const Rows<float*> o = rows_of (out, nchan, npol);
      status (dspsr_amd_sk_mask (handle, i.base, i.cs, i.ps, o.base, o.cs, o.ps), "HIP::SpectralKurtosisEngine::mask");
    }

    //! the call is commented out in the reference (SpectralKurtosis.C:231)
    void insertsk (const dsp::TimeSeries*, dsp::TimeSeries*, unsigned) { }

    dspsr_amd_sk* get_handle () const { return handle; }

  protected:
    void status (int code, const char* method) { check (ctx, code, method, "no context"); }
    void options (const char* method)
    { status (dspsr_amd_sk_set_options (handle, std_devs, chan_start, chan_end == nchan ? 0 : chan_end, 0, 0, 0), method); }
    void fetch_mask (const char* method)
    {
      host_mask.resize (size_t (dspsr_amd_sk_npart (handle)) * nchan + 1);       // (one spare element: never empty)
      status (dspsr_amd_copy (ctx, &host_mask[0], dspsr_amd_sk_zapmask_dev (handle), host_mask.size () - 1, DSPSR_AMD_D2H), method);
    }
    dspsr_amd_ctx* ctx;
    dspsr_amd_sk* handle;
    unsigned std_devs, chan_start, chan_end, nchan, npol;
    std::vector<float> host_estimates;
    std::vector<unsigned char> host_mask;
  };
}

#endif
