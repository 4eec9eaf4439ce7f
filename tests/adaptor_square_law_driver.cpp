// What the adaptors make of DSPSR's engine calls when Detection is a square law (dspsr -d 1, -d 2, one input polarisation),
// without a GPU: the pipeline Filterbank -> Detection::square_law (out of place) -> Fold of tests/adaptor_trace_driver.cpp over
// the recording C-ABI of tests/capi_recorder.cpp, one log -- the ordered C-ABI calls with their arguments, the Errors, the
// counters of the HIP::Chain.  tests/test_adaptor_square_law_host.py compares it with tests/golden/adaptor_square_law/chain_square_law.txt.
//   adaptor_square_law_driver FILE
#include <stdio.h>
#include <string.h>

#include <string>

#include "dspsr_amd_engines.h"
#include "capi_recorder.h"

static void note_error (const Error& e)
{ rec::note ("Error %s: %s", e.code == InvalidParam ? "InvalidParam" : "InvalidState", e.message.c_str ()); }

#define DO(stmt) do { rec::note ("%s", "# " #stmt); try { stmt; } catch (Error& e) { note_error (e); } } while (0)

static dsp::TimeSeries* series (dsp::Memory* memory, unsigned nchan, unsigned npol, unsigned ndim, uint64_t ndat, Signal::State state)
{
  dsp::TimeSeries* t = new dsp::TimeSeries;
  t->set_nchan (nchan); t->set_npol (npol); t->set_ndim (ndim); t->set_state (state); t->set_rate (1e6);
  if (memory) t->set_memory (memory);
  t->resize (ndat);
  return t;
}

static const unsigned NPART = 3, NKEEP = 8, NBIN = 8, NCHAN = 4;
static const uint64_t STEP = 40, NDAT_IN = NPART * STEP + 16, NDAT = NPART * NKEEP;

struct Pipeline
{
  dspsr_amd_ctx* ctx;
  dsp::Memory* dmem;
  HIP::Chain* chain;
  dsp::TimeSeries* in;
  dsp::TimeSeries* chan;                         // the channelised block
  dsp::TimeSeries* det_out;                      // the detected block: npol_out x ndim 1
  dsp::Response response;
  dsp::Filterbank filterbank;
  HIP::FilterbankEngine* fbe;
  HIP::DetectionEngine* det;
  HIP::FoldEngine* eng;
  dsp::Fold fold;

  Pipeline (bool deferred, unsigned npol, Signal::State state, unsigned npol_out)
  {
    ctx = 0;
    dspsr_amd_ctx_create (0, DSPSR_AMD_NEW_STREAM, &ctx);
    dmem = new HIP::DeviceMemory (ctx);
    chain = new HIP::Chain (ctx);
    chain->set_deferred (deferred);
    in = series (dmem, 1, npol, 1, NDAT_IN, Signal::Nyquist);
    in->set_input_sample (1000);
    chan = series (dmem, NCHAN, npol, 2, NDAT, Signal::Analytic);
    det_out = series (dmem, NCHAN, npol_out, 1, NDAT, state);
    response.impulse_pos = 3; response.impulse_neg = 5; response.nchan = NCHAN; response.ndat = 16;
    response.kernel.resize (2 * NCHAN * 16);
    filterbank.nchan_subband = NCHAN; filterbank.freq_res = 16; filterbank.input = in; filterbank.response = &response;
    rec::set_step (STEP);
    rec::set_fold (2, NDAT);
    fbe = new HIP::FilterbankEngine (ctx, chain);
    DO (fbe->setup (&filterbank));
    det = new HIP::DetectionEngine (ctx, chain);
    eng = new HIP::FoldEngine (ctx, chain);
    fold.set_input (det_out); fold.set_engine (eng); fold.set_nbin (NBIN);
  }
  void perform () { DO (fbe->perform (in, chan, NPART, STEP, 2 * NKEEP)); }
  void detect () { DO (det->square_law (chan, det_out)); }
  void fold_whole () { DO (fold.prepare_output ()); DO (fold.fold (0.25, 37.5e-6, 0, NDAT)); }
  void block () { perform (); detect (); fold_whole (); }
  void counters ()
  {
    rec::note ("chain: fused %llu, eager %llu, dropped %llu, nfold %u, deferred %d", (unsigned long long) chain->get_fused_blocks (),
               (unsigned long long) chain->get_eager_blocks (), (unsigned long long) chain->get_dropped_blocks (), chain->get_nfold (),
               (int) chain->get_deferred ());
  }
  void result () { DO (fold.get_result ()); counters (); }
};

static void scenario ()
{
  rec::note ("## Intensity, deferred: perform and square_law recorded, fold launches perform_fold with state 2");
  { Pipeline p (true, 2, Signal::Intensity, 1); p.block (); p.block (); p.result (); }
  rec::note ("## PPQQ, deferred: state 3");
  { Pipeline p (true, 2, Signal::PPQQ, 2); p.block (); p.result (); }
  rec::note ("## one input polarisation, deferred: the power of that polarisation, state 2");
  { Pipeline p (true, 1, Signal::Intensity, 1); p.block (); p.result (); }
  rec::note ("## eager chain: the three launches");
  { Pipeline p (false, 2, Signal::PPQQ, 2); p.block (); p.result (); }
  rec::note ("## deferred, finish() between perform and square_law: the filterbank runs, square_law and fold are launches of their own");
  { Pipeline p (true, 2, Signal::Intensity, 1); p.perform (); DO (p.fbe->finish ()); p.detect (); p.fold_whole (); p.result (); }
  rec::note ("## deferred, a fold of a piece of the block: everything recorded runs, then the eager fold");
  {
    Pipeline p (true, 2, Signal::PPQQ, 2);
    p.perform (); p.detect ();
    DO (p.fold.prepare_output ()); DO (p.fold.fold (0.25, 37.5e-6, 0, NDAT / 2));
    p.result ();
  }
  rec::note ("## deferred, an output state the fused fold does not write (Coherence rows asked of square_law): eager");
  { Pipeline p (true, 2, Signal::Coherence, 2); p.block (); p.result (); }
  rec::note ("## deferred, a profile shape that does not go with the state (PPQQ folded as npol 1): eager");
  {
    Pipeline p (true, 2, Signal::PPQQ, 2);
    dsp::TimeSeries* other = series (p.dmem, NCHAN, 1, 1, NDAT, Signal::Intensity);
    p.perform (); p.detect ();
    p.fold.set_input (other);
    p.fold_whole ();
    p.result ();
  }
  rec::note ("## deferred, a reader of the detected rows of a fused block: refused");
  {
    Pipeline p (true, 2, Signal::Intensity, 1);
    p.block ();
    dsp::TimeSeries* again = series (p.dmem, NCHAN, 1, 1, NDAT, Signal::Intensity);
    DO (p.det->square_law (p.chan, again));
    p.result ();
  }
}

int main (int argc, char** argv)
{
  if (argc != 2) { fprintf (stderr, "usage: %s FILE\n", argv[0]); return 2; }
  rec::reset ();
  try { scenario (); }
  catch (Error& e) { rec::note ("the scenario ended with:"); note_error (e); }
  FILE* fp = fopen (argv[1], "w");
  if (!fp) { fprintf (stderr, "cannot write %s\n", argv[1]); return 2; }
  fputs (rec::text ().c_str (), fp);
  fclose (fp);
  return 0;
}
