// dspsr_amd_cyclic_engine.h -- HIP::CyclicFoldEngine: dsp::CyclicFoldEngine (Signal/Pulsar/dsp/CyclicFold.h:93-163) over the
// C-ABI of include/dspsr_amd.h (dspsr_amd_cyclic_fold_*), the twin of CUDA::CyclicFoldEngineCUDA (CyclicFoldEngineCUDA.cu).
//
// The lag products are folded on the device.  synch() copies the device lag data into the base class's `lagdata` (the same
// [bin][pol][chan][lag][re, im] order, CyclicFold.C:329-337) and calls the base class's synch, which windows and transforms
// them into the output PhaseSeries on the host -- what the CUDA engine does (CyclicFoldEngineCUDA.cu:72-107).  The input
// TimeSeries lives on the device (HIP::DeviceMemory); the output PhaseSeries and `lagdata` on the host.
// Installed where the CUDA engine is (LoadToFold1.C:1010-1030):  fold->set_engine (new HIP::CyclicFoldEngine (ctx));
#ifndef DSPSR_AMD_CYCLIC_ENGINE_H
#define DSPSR_AMD_CYCLIC_ENGINE_H

#include <string.h>

#include "dsp/CyclicFold.h"

#include "dspsr_amd_adaptor_common.h"   // HIP::check, HIP::rows_of

namespace HIP
{
  class CyclicFoldEngine : public dsp::CyclicFoldEngine
  {
  public:
    CyclicFoldEngine (dspsr_amd_ctx* _ctx) : ctx (_ctx), handle (0)
    {
      status (dspsr_amd_cyclic_fold_create (ctx, &handle), "HIP::CyclicFoldEngine");
      use_set_bins = false;                                   // Fold::fold drives set_bin sample by sample (Fold.C:744-787)
    }
    ~CyclicFoldEngine () { if (handle) dspsr_amd_cyclic_fold_destroy (handle); }

    // the base class keeps the values (and, in DSPSR, the lag-to-channel plan that its synch uses)
    void set_nlag (unsigned _nlag) { dsp::CyclicFoldEngine::set_nlag (_nlag); }
    void set_mover (unsigned _mover) { dsp::CyclicFoldEngine::set_mover (_mover); }
    void set_nbin (unsigned _nbin) { dsp::CyclicFoldEngine::set_nbin (_nbin); }
    void set_npol (unsigned _npol) { dsp::CyclicFoldEngine::set_npol (_npol); }

    //! CyclicFold.C:234-281: the shape is complete here; the device lag array and the host copy are sized (and zeroed when new)
    void set_ndat (uint64_t _ndat, uint64_t _idat_start)
    {
      setup ();
      if (ndim != 2)
        throw Error (InvalidState, "HIP::CyclicFoldEngine::set_ndat", "Only Analytic input data is currently supported");
      status (dspsr_amd_cyclic_fold_set_shape (handle, nchan, npol, npol_out, nlag, mover, nbin), "HIP::CyclicFoldEngine::set_ndat");
      status (dspsr_amd_cyclic_fold_set_ndat (handle, _ndat, _idat_start), "HIP::CyclicFoldEngine::set_ndat");
      ndat_fold = (unsigned) _ndat;
      idat_start = _idat_start;
      const uint64_t need = uint64_t (nlag) * nbin * npol_out * ndim * nchan;
      if (need > lagdata_size) {
        delete [] lagdata;
        lagdata = new float [need];
        lagdata_size = need;
        memset (lagdata, 0, sizeof (float) * lagdata_size);
      }
    }

    void set_bin (uint64_t idat, double ibin, double bins_per_samp)
    { status (dspsr_amd_cyclic_fold_set_bin (handle, idat, ibin, bins_per_samp), "HIP::CyclicFoldEngine::set_bin"); }

    void fold ()
    {
      setup ();
      const dsp::TimeSeries* in = parent->get_input ();
      if (in->get_memory ()->on_host ())
        throw Error (InvalidState, "HIP::CyclicFoldEngine::fold", "the input TimeSeries is not in device memory");
      const Rows<const float*> rows = rows_of (in, nchan, npol);      // the shape Fold::Engine::setup read from this input
      status (dspsr_amd_cyclic_fold_fold (handle, rows.base, rows.cs, rows.ps), "HIP::CyclicFoldEngine::fold");
      synchronized = false;
    }

    void zero ()
    {
      dsp::CyclicFoldEngine::zero ();                         // the output profiles and the host lag data
      status (dspsr_amd_cyclic_fold_zero (handle), "HIP::CyclicFoldEngine::zero");
    }

    void synch (dsp::PhaseSeries* to)
    {
      if (synchronized) return;
      if (!lagdata)
        throw Error (InvalidState, "HIP::CyclicFoldEngine::synch", "no lag data (set_ndat was never called)");
      status (dspsr_amd_cyclic_fold_synch_lags (handle, lagdata), "HIP::CyclicFoldEngine::synch");
      dsp::CyclicFoldEngine::synch (to);
    }

    //! the host copy of the lag data as of the last synch
    const float* get_lagdata () const { return lagdata; }
    uint64_t get_lagdata_size () const { return lagdata_size; }

  protected:
    void status (int code, const char* method) { check (ctx, code, method); }
    dspsr_amd_ctx* ctx;
    dspsr_amd_cyclic_fold* handle;
  };
}

#endif
