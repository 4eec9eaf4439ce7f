// FUNCTIONAL MINIATURE (see ../Error.h): dsp::CyclicFold and dsp::CyclicFoldEngine with the members and virtual signatures
// declared in Signal/Pulsar/dsp/CyclicFold.h:38-163.  The bodies restate what include/dspsr_amd.h states of
// Signal/Pulsar/CyclicFold.C (prepare :30-54, prepare_output :69-154, set_ndat :234-281, set_bin :293-301, fold :339-448,
// synch :450-555); the backward complex-to-real transform that the real class asks of PSRCHIVE's FTransform (bcr1d,
// unnormalised) is a plain double sum here.  dsp::Fold::prepare_output is not virtual in the miniature dsp/Fold.h, so a
// driver calls CyclicFold::prepare_output on the CyclicFold itself.
#pragma once
#include <string.h>
#include "dsp/Fold.h"
namespace dsp {
  class CyclicFoldEngine : public Fold::Engine {
  public:
    CyclicFoldEngine () : out (0), nlag (0), mover (1), nbin (0), npol_out (0), binplan_size (0), lagdata (0), lagdata_size (0)
    { binplan[0] = binplan[1] = 0; }
    ~CyclicFoldEngine () { delete [] binplan[0]; delete [] binplan[1]; delete [] lagdata; }
    virtual void set_nlag (unsigned _nlag) { nlag = _nlag; }
    virtual void set_mover (unsigned _mover) { mover = _mover; }
    virtual void set_nbin (unsigned _nbin) { nbin = _nbin; }
    virtual void set_npol (unsigned _npol) { npol_out = _npol; }
    virtual void set_bin (uint64_t idat, double ibin, double bins_per_samp)
    {
      binplan[0][idat - idat_start] = unsigned (ibin);
      binplan[1][idat - idat_start] = unsigned (ibin + 0.5 * bins_per_samp) % nbin;
    }
    uint64_t set_bins (double, double, uint64_t, uint64_t) { return 0; }
    uint64_t get_bin_hits (int) { return 0; }
    virtual PhaseSeries* get_profiles () { return out; }
    void set_profiles (PhaseSeries* _out) { out = _out; }
    virtual void fold ()
    {
      setup ();
      if (ndat_fold <= nlag) return;
      const TimeSeries* in = parent->get_input ();
      const unsigned npol_in = in->get_npol ();
      for (unsigned ichan = 0; ichan < nchan; ichan++) {
        const float* p[2];
        for (unsigned ipol = 0; ipol < npol_in; ipol++) p[ipol] = in->get_datptr (ichan, ipol) + 2 * idat_start;
        for (uint64_t idat = 0; idat < ndat_fold - nlag; idat++)
          for (unsigned ilag = 0; ilag < nlag; ilag++) {
            const unsigned ibin = binplan[ilag % 2][idat + ilag / 2];
            const uint64_t a = 2 * idat, b = 2 * (idat + ilag);
            mac (get_lagdata_ptr (ichan, 0, ibin) + 2 * ilag, p[0] + a, p[0] + b);
            if (npol_in == 2) mac (get_lagdata_ptr (ichan, npol_out == 1 ? 0 : 1, ibin) + 2 * ilag, p[1] + a, p[1] + b);
            if (npol_out == 4) {
              mac (get_lagdata_ptr (ichan, 2, ibin) + 2 * ilag, p[0] + a, p[1] + b);
              mac (get_lagdata_ptr (ichan, 3, ibin) + 2 * ilag, p[1] + a, p[0] + b);
            }
          }
      }
      synchronized = false;
    }
    virtual void synch (PhaseSeries* to)
    {
      if (synchronized) return;
      const unsigned n = 2 * nlag - 2, keep = n / mover;
      for (unsigned ibin = 0; ibin < nbin; ibin++)
        for (unsigned ipol = 0; ipol < npol_out; ipol++)
          for (unsigned ichan = 0; ichan < nchan; ichan++) {
            float* lags = get_lagdata_ptr (ichan, ipol, ibin);
            if (mover > 1)
              for (unsigned ilag = 1; ilag < nlag; ilag++) {
                float x = (M_PI / 3) * mover * ilag / ((float) (2 * nlag - 2));
                float y = 0.5 * (1 + cos (2 * M_PI * float (ilag) / float (2 * nlag)));
                float f = y * sinf (x) / x;
                lags[2 * ilag] *= f;
                lags[2 * ilag + 1] *= f;
              }
            for (unsigned schan = 0; schan < keep; schan++) {
              const unsigned j = schan * mover;              // out[j] = sum over the Hermitian spectrum of z[k] e^{+2 pi i j k / n}
              double s = lags[0] + ((j & 1) ? -1.0 : 1.0) * lags[2 * (nlag - 1)];
              for (unsigned k = 1; k + 1 < nlag; k++) {
                const double ph = 2.0 * M_PI * double ((uint64_t (j) * k) % n) / n;
                s += 2.0 * (lags[2 * k] * cos (ph) - lags[2 * k + 1] * sin (ph));
              }
              to->get_datptr (ichan * keep + schan, ipol)[ibin] = float (s);
            }
          }
      synchronized = true;
    }
    virtual void zero ()
    {
      get_profiles ()->zero ();
      if (lagdata && lagdata_size > 0) memset (lagdata, 0, sizeof (float) * lagdata_size);
    }
    virtual void set_ndat (uint64_t _ndat, uint64_t _idat_start)
    {
      setup ();
      if (_ndat > binplan_size) {
        delete [] binplan[0]; delete [] binplan[1];
        binplan[0] = new unsigned [_ndat]; binplan[1] = new unsigned [_ndat];
        binplan_size = _ndat;
      }
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
    uint64_t get_ndat_folded () const { return 0; }
  protected:
    PhaseSeries* out;
    unsigned nlag, mover, nbin, npol_out;
    unsigned* binplan[2];
    uint64_t binplan_size;
    float* lagdata;
    uint64_t lagdata_size;
    float* get_lagdata_ptr (unsigned ichan, unsigned ipol, unsigned ibin)     // [bin][pol][chan][lag][re, im]
    { return lagdata + ndim * ((uint64_t (ibin) * npol_out + ipol) * nchan * nlag + uint64_t (ichan) * nlag); }
    static void mac (float* d, const float* a, const float* b)
    { d[0] += a[0] * b[0] + a[1] * b[1]; d[1] += a[1] * b[0] - a[0] * b[1]; }
  };
  class CyclicFold : public Fold {
  public:
    CyclicFold () : nlag (0), mover (1), npol (0) {}
    virtual ~CyclicFold () {}
    virtual void prepare ()
    {
      if (!engine) set_engine (new CyclicFoldEngine);
      CyclicFoldEngine* cfe = dynamic_cast<CyclicFoldEngine*> (engine.get ());
      if (!cfe) throw Error (InvalidState, "dsp::CyclicFold:prepare", "Folding engine is not a CyclicFoldEngine");
      cfe->set_nlag (nlag);
      cfe->set_mover (mover);
      cfe->set_npol (npol);
      cfe->set_profiles (output);
    }
    void set_nlag (unsigned _nlag) { nlag = _nlag; }
    unsigned get_nlag () const { return nlag; }
    void set_mover (unsigned _mover) { mover = _mover; }
    unsigned get_mover () const { return mover; }
    void set_nchan (unsigned nchan) { set_nlag (mover * nchan / 2 + 1); }
    void set_npol (unsigned _npol) { npol = _npol; }
    unsigned get_npol () const { return npol; }
    virtual void prepare_output ()                             // first use: the output takes the cyclic shape, zeroed
    {
      PhaseSeries* o = get_output ();
      if (o->integration_length != 0.0) return;
      const double length = o->integration_length;
      const uint64_t total = o->ndat_total;
      o->Observation::copy_configuration (input);
      o->set_nchan ((2 * nlag - 2) / mover * input->get_nchan ());
      o->set_npol (npol);
      o->set_ndim (1);
      // (the miniature Signal::State has no PP_State: one input polarisation is Intensity here too)
      o->set_state (npol == 1 ? Signal::Intensity : npol == 2 ? Signal::PPQQ : Signal::Coherence);
      o->resize (folding_nbin);
      o->zero ();
      o->integration_length = length;
      o->ndat_total = total;
    }
  protected:
    unsigned nlag, mover, npol;
  };
}
