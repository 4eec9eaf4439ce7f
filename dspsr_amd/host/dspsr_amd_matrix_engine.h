// dspsr_amd_matrix_engine.h -- HIP::MatrixFilterbankEngine: HIP::FilterbankEngine for a dsp::Filterbank whose response may be
// a matrix response (`dspsr -pac`: PolnCalibration x Dedispersion as a ResponseProduct, LoadToFold1.C:270-289).
//
// dsp::Filterbank decides matrix_convolution = response->get_ndim () == 8 in make_preparations (Filterbank.C:186-206) and its
// CPU loop then calls Response::operate (data1, data2) (Filterbank.C:574-656, Response.C:515-585); the reference's CUDA engine
// copies ndat * nchan complex numbers whatever ndim is (FilterbankCUDA.cu:73-168).  This engine reads get_ndim ():
//   8  the response goes to dspsr_amd_filterbank_set_response_matrix -- response->get_datptr (0, 0) holds nchan * ndat matrices
//      of 8 floats in the order f11, f21, f22, f12 (Response.C:614-640), which is the library's order; the reference's two
//      errors (Filterbank.C:199-205) are thrown here as it throws them;
//   2  HIP::FilterbankEngine::setup, unchanged.
// perform, finish, the raw-input side channel and the Chain are the base class's.
// Installed where the CUDA engine is (FilterbankConfig.C:102-130):  filterbank->set_engine (new HIP::MatrixFilterbankEngine (ctx));
#ifndef DSPSR_AMD_MATRIX_ENGINE_H
#define DSPSR_AMD_MATRIX_ENGINE_H

#include "dspsr_amd_engines.h"

namespace HIP
{
  class MatrixFilterbankEngine : public FilterbankEngine
  {
  public:
    MatrixFilterbankEngine (dspsr_amd_ctx* _ctx, Chain* _chain = 0) : FilterbankEngine (_ctx, _chain) { }

    void setup (dsp::Filterbank* filterbank)
    {
      const unsigned ndim = filterbank->has_response () ? filterbank->get_response ()->get_ndim () : 2;
      if (ndim != 8)
      {
        if (ndim != 2)
          throw Error (InvalidState, "HIP::MatrixFilterbankEngine::setup", "response ndim=%u is neither 2 (complex) nor 8 (Jones)", ndim);
        FilterbankEngine::setup (filterbank);
        return;
      }
      const dsp::TimeSeries* input = filterbank->get_input ();
      if (input->get_nchan () > 1)                                              // Filterbank.C:199-201
        throw Error (InvalidState, "dsp::Filterbank::make_preparations", "matrix convolution untested for > one input channel");
      if (input->get_npol () != 2)                                              // Filterbank.C:203-205
        throw Error (InvalidState, "dsp::Filterbank::make_preparations", "matrix convolution and input.npol != 2");
      filterbank->set_passband (NULL);          // the engine does not maintain the passband
      if (chain) chain->flush ();
      replace (filterbank, filterbank->get_response (), true, "HIP::MatrixFilterbankEngine::setup");
    }

    //! Response::get_ndim of what the library object holds: 0 none, 2 complex, 8 Jones
    int response_ndim () const { return dspsr_amd_filterbank_response_ndim (fb); }
  };
}

#endif
