// Drives every adaptor class of dspsr_amd/host over the recording C-ABI of tests/capi_recorder.cpp (no GPU, no -ldspsr_amd) and
// writes, per scenario, the ordered list of C-ABI calls with their arguments, the Errors thrown and the counters of the
// HIP::Chain: the behaviour of the adaptors as the library sees it.  Nothing is computed, so the shapes are tiny.
//   adaptor_trace_driver DIR      writes DIR/<scenario>.txt            (tests/test_adaptor_trace_host.py compares them with
//                                                                        tests/golden/adaptor_trace/)
//   adaptor_trace_driver --messages   checks that a library message holding a printf conversion reaches the Error verbatim
// A line "# statement" is the driver's call, the lines after it what the adaptors made of it.
#include <stdio.h>
#include <string.h>

#include <string>

#include "dspsr_amd_matrix_engine.h"
#include "dspsr_amd_cyclic_engine.h"
#include "dspsr_amd_sk_engine.h"
#include "capi_recorder.h"

static void note_error (const Error& e)
{ rec::note ("Error %s: %s", e.code == InvalidParam ? "InvalidParam" : "InvalidState", e.message.c_str ()); }

#define DO(stmt) do { rec::note ("%s", "# " #stmt); try { stmt; } catch (Error& e) { note_error (e); } } while (0)

static dspsr_amd_ctx* new_ctx ()
{
  dspsr_amd_ctx* ctx = 0;
  dspsr_amd_ctx_create (0, DSPSR_AMD_NEW_STREAM, &ctx);
  return ctx;
}

static dsp::TimeSeries* series (dsp::Memory* memory, unsigned nchan, unsigned npol, unsigned ndim, uint64_t ndat, Signal::State state)
{
  dsp::TimeSeries* t = new dsp::TimeSeries;
  t->set_nchan (nchan); t->set_npol (npol); t->set_ndim (ndim); t->set_state (state); t->set_rate (1e6);
  if (memory) t->set_memory (memory);
  t->resize (ndat);
  return t;
}

static void counters (const HIP::Chain* chain)
{
  rec::note ("chain: fused %llu, eager %llu, dropped %llu, nfold %u, deferred %d, drop_unfolded %d",
             (unsigned long long) chain->get_fused_blocks (), (unsigned long long) chain->get_eager_blocks (),
             (unsigned long long) chain->get_dropped_blocks (), chain->get_nfold (), (int) chain->get_deferred (),
             (int) chain->get_drop_unfolded ());
}

// ---- the fold pipeline of one thread: Filterbank -> Detection (in place, LoadToFold1.C:545-546) -> Fold
static const unsigned NPART = 3, NKEEP = 8, NBIN = 8;
static const uint64_t STEP = 40, NDAT_IN = NPART * STEP + 16, NDAT = NPART * NKEEP;

struct Pipeline
{
  dspsr_amd_ctx* ctx;
  dsp::Memory* dmem;
  HIP::Chain* chain;
  dsp::TimeSeries* in;                           // float rows in front of the filterbank
  dsp::TimeSeries* chan;                         // the channelised block, detected in place
  dsp::Response response;
  dsp::Filterbank filterbank;
  HIP::FilterbankEngine* fbe;
  HIP::DetectionEngine* det;
  HIP::FoldEngine* eng;
  dsp::Fold fold;

  Pipeline (bool with_chain, bool deferred, unsigned nchan = 4, unsigned npol = 2)
  {
    ctx = new_ctx ();
    dmem = new HIP::DeviceMemory (ctx);
    chain = with_chain ? new HIP::Chain (ctx) : 0;
    if (chain) chain->set_deferred (deferred);
    in = series (dmem, 1, npol, 1, NDAT_IN, Signal::Nyquist);
    in->set_input_sample (1000);
    chan = series (dmem, nchan, npol, 2, NDAT, Signal::Analytic);
    response.impulse_pos = 3; response.impulse_neg = 5; response.nchan = nchan; response.ndat = 16;
    response.kernel.resize (2 * nchan * 16);
    filterbank.nchan_subband = nchan; filterbank.freq_res = 16; filterbank.input = in; filterbank.response = &response;
    rec::set_step (STEP);
    rec::set_fold (2, NDAT);
    fbe = new HIP::FilterbankEngine (ctx, chain);
    DO (fbe->setup (&filterbank));
    det = new HIP::DetectionEngine (ctx, chain);
    eng = new HIP::FoldEngine (ctx, chain);
    fold.set_input (chan); fold.set_engine (eng); fold.set_nbin (NBIN);
  }
  void perform () { DO (fbe->perform (in, chan, NPART, STEP, 2 * NKEEP)); }
  void detect () { DO (det->polarimetry (2, chan, chan)); }
  void fold_whole () { DO (fold.prepare_output ()); DO (fold.fold (0.25, 37.5e-6, 0, NDAT)); }
  void block () { perform (); detect (); fold_whole (); }
  void result () { DO (fold.get_result ()); counters_if (); }
  void counters_if () { if (chain) counters (chain); }
};

static void chain_none ()
{
  Pipeline p (false, false);
  p.block ();
  DO (p.fbe->finish ());
  p.block ();
  DO (p.fbe->perform (p.in, 0, NPART, STEP, 2 * NKEEP));                       // out == NULL: benchmark only
  dsp::BitSeries* raw = new dsp::BitSeries;
  raw->set_memory (p.dmem); raw->resize (NDAT_IN, 2);
  DO (p.fbe->set_raw_input (raw->get_rawptr (), NDAT_IN, 1000, DSPSR_AMD_RAW_GENERIC, 0.5f));
  p.perform ();                                                                 // the packed block stands in
  p.perform ();                                                                 // one shot: float rows again
  DO (p.fbe->set_raw_input (raw->get_rawptr (), NDAT_IN, 1000, DSPSR_AMD_RAW_GENERIC, 0.5f));
  DO (p.fbe->perform (p.in, 0, NPART, STEP, 2 * NKEEP));                       // a matching block and out == NULL
  DO (p.fbe->perform_raw ((const int8_t*) raw->get_rawptr (), DSPSR_AMD_RAW_CASPSR, 0.25f, p.chan, NPART, 2 * NKEEP));
  dsp::BitSeries host_bits;
  host_bits.resize (NDAT_IN, 2); host_bits.set_input_sample (1000);
  DO (HIP::transfer_bitseries (p.ctx, &host_bits, raw, p.fbe, DSPSR_AMD_RAW_GENERIC, 0.125f));
  p.perform ();
  DO (p.det->square_law (p.chan, p.chan));
  p.result ();
  DO (p.fold.reset ());
  DO (p.eng->get_ndat_folded ());
  DO (delete p.eng);
  DO (delete p.fbe);
}

static void chain_eager ()
{
  Pipeline p (true, false);
  p.block ();
  DO (p.fbe->finish ());
  p.block ();
  p.result ();
}

static void chain_deferred_float ()
{
  Pipeline p (true, true);
  p.block ();
  p.block ();
  p.result ();
  DO (p.fold.reset ());
  p.block ();
  p.result ();
}

static void chain_deferred_raw ()
{
  Pipeline p (true, true);
  dsp::BitSeries* raw = new dsp::BitSeries;
  raw->set_memory (p.dmem); raw->resize (NDAT_IN, 2);
  rec::note ("## matching input: accepted");
  DO (p.fbe->set_raw_input (raw->get_rawptr (), NDAT_IN, 1000, DSPSR_AMD_RAW_GENERIC, 0.5f));
  p.block ();
  rec::note ("## mismatched input_sample: float rows");
  DO (p.fbe->set_raw_input (raw->get_rawptr (), NDAT_IN, 1001, DSPSR_AMD_RAW_GENERIC, 0.5f));
  p.block ();
  rec::note ("## mismatched ndat: float rows");
  DO (p.fbe->set_raw_input (raw->get_rawptr (), NDAT_IN - 1, 1000, DSPSR_AMD_RAW_GENERIC, 0.5f));
  p.block ();
  rec::note ("## mismatched in_step: float rows");
  DO (p.fbe->set_raw_input (raw->get_rawptr (), NDAT_IN, 1000, DSPSR_AMD_RAW_GENERIC, 0.5f));
  rec::set_step (STEP + 1);
  p.block ();
  rec::set_step (STEP);
  rec::note ("## the block of the refused hand-over is not kept for the next perform");
  p.block ();
  rec::note ("## matching input, executed eagerly by finish");
  DO (p.fbe->set_raw_input (raw->get_rawptr (), NDAT_IN, 1000, DSPSR_AMD_RAW_CASPSR, 0.25f));
  p.perform ();
  DO (p.fbe->finish ());
  p.detect (); p.fold_whole ();
  p.result ();
}

static void chain_finish_each ()
{
  Pipeline p (true, true);
  for (int b = 0; b < 2; b++)
  {
    p.perform ();
    DO (p.fbe->finish ());
    p.detect (); p.fold_whole ();
  }
  p.result ();
}

static void chain_pieces ()
{
  Pipeline p (true, true);
  p.block ();
  p.perform (); p.detect ();
  DO (p.fold.prepare_output ());
  DO (p.fold.fold (0.25, 37.5e-6, 0, 10));                                       // a sub-integration boundary inside the block
  DO (p.fold.fold (0.75, 37.5e-6, 10, NDAT - 10));
  p.perform (); p.detect ();
  DO (p.fold.fold (0.25, 37.5e-6, 4, NDAT - 4));                                 // one piece that does not start the block
  p.result ();
}

static void chain_two_folds ()
{
  Pipeline p (true, true);
  dsp::Fold fold2;
  HIP::FoldEngine* eng2 = new HIP::FoldEngine (p.ctx, p.chain);
  fold2.set_input (p.chan); fold2.set_engine (eng2); fold2.set_nbin (NBIN / 2);
  for (int b = 0; b < 2; b++)
  {
    p.block ();
    DO (fold2.prepare_output ());
    DO (fold2.fold (0.5, 23.25e-6, 0, NDAT));
  }
  p.result ();
  DO (fold2.get_result ());
  DO (delete eng2);                                                               // one Fold left: the next block fuses
  p.block ();
  p.result ();
}

static void chain_zeroed ()
{
  Pipeline p (true, true);
  p.chan->set_zeroed_data (true);
  p.eng->get_profiles ()->set_hits_nchan (p.chan->get_nchan ());
  p.block ();
  p.block ();
  p.result ();
  DO (p.fold.reset ());
  rec::note ("## nchan * nbin changes: the device hits are reallocated");
  p.fold.set_nbin (NBIN / 2);
  p.block ();
  p.result ();
  DO (p.eng->zero ());
  DO (p.eng->synch (p.fold.get_result ()));
  rec::note ("## hits of one channel only: the plain fold, fused");
  p.eng->get_profiles ()->set_hits_nchan (1);
  p.block ();
  p.result ();
  DO (delete p.eng);
}

static void chain_unfolded ()
{
  Pipeline p (true, true);
  p.perform (); p.detect ();                                                      // no Fold for this block (Subint.h:270)
  p.block ();
  p.counters_if ();
  p.perform ();                                                                   // a block without detection either
  DO (p.chain->set_drop_unfolded (false));
  p.block ();
  p.counters_if ();
  p.perform (); p.detect ();
  p.block ();                                                                     // (the Error left nothing pending)
  p.result ();
}

static void chain_refused_readers ()
{
  Pipeline p (true, true);
  HIP::TimeSeriesEngine tse (p.ctx, p.chain);
  dsp::TimeSeries* kept = series (p.dmem, 4, 2, 2, NDAT, Signal::Analytic);
  DO (tse.prepare (kept));
  p.block ();
  DO (tse.copy_data_fpt (p.chan, 2, 5));
  DO (p.det->polarimetry (2, p.chan, kept));
  DO (p.det->square_law (p.chan, kept));
  dsp::Fold outsider;
  HIP::FoldEngine* eng2 = new HIP::FoldEngine (p.ctx);                            // not on the chain
  outsider.set_input (p.chan); outsider.set_engine (eng2); outsider.set_nbin (NBIN);
  DO (outsider.prepare_output ());
  DO (outsider.fold (0.5, 23.25e-6, 0, NDAT));
  DO (p.fold.fold (0.25, 37.5e-6, 0, NDAT));                                      // the chain's own Fold, a second time
  rec::note ("## a reader of a block that is only recorded: executed first");
  p.perform (); p.detect ();
  DO (tse.copy_data_fpt (p.chan, 0, NDAT));
  p.fold_whole ();
  p.perform ();
  DO (tse.prepare (p.chan));
  DO (tse.copy_data_fpt (kept, 0, 4));                                            // the recorded output is the copy's target
  p.detect (); p.fold_whole ();
  rec::note ("## the next perform lifts the refusal");
  p.block ();
  p.perform ();
  DO (tse.prepare (kept));
  DO (tse.copy_data_fpt (p.chan, 0, 4));
  p.result ();
}

static void chain_pending ()
{
  Pipeline p (true, true);
  rec::note ("## set_deferred (false) with a block pending");
  p.perform (); p.detect ();
  DO (p.chain->set_deferred (false));
  p.fold_whole ();
  p.counters_if ();
  DO (p.chain->set_deferred (true));
  rec::note ("## setup () with a block pending");
  p.perform (); p.detect ();
  DO (p.fbe->setup (&p.filterbank));
  p.fold_whole ();
  p.counters_if ();
  rec::note ("## perform with out == NULL, a block pending");
  p.perform (); p.detect ();
  DO (p.fbe->perform (p.in, 0, NPART, STEP, 2 * NKEEP));
  p.fold_whole ();
  p.counters_if ();
  rec::note ("## ~FilterbankEngine with a block pending");
  p.perform (); p.detect ();
  DO (delete p.fbe);
  p.fold_whole ();
  p.counters_if ();
  rec::note ("## ~FilterbankEngine with a filterbank call pending only");
  p.fbe = new HIP::FilterbankEngine (p.ctx, p.chain);
  DO (p.fbe->setup (&p.filterbank));
  p.perform ();
  DO (delete p.fbe);
  p.detect (); p.fold_whole ();
  p.result ();
}

static void chain_detected_shapes ()
{
  Pipeline p (true, true);
  dsp::TimeSeries* stokes = series (p.dmem, 4, 1, 4, NDAT, Signal::Coherence);
  dsp::TimeSeries* intensity = series (p.dmem, 4, 4, 1, NDAT, Signal::Coherence);
  rec::note ("## ndim 4, Stokes through set_output_state, out of place: fused");
  p.fold.set_input (stokes);
  DO (p.det->set_output_state (Signal::Stokes));
  p.perform ();
  DO (p.det->polarimetry (4, p.chan, stokes));
  p.fold_whole ();
  rec::note ("## ndim 4, the state read from the output");
  DO (p.det = new HIP::DetectionEngine (p.ctx, p.chain));
  p.perform ();
  DO (p.det->polarimetry (4, p.chan, stokes));
  p.fold_whole ();
  stokes->set_state (Signal::Stokes);
  p.perform ();
  DO (p.det->polarimetry (4, p.chan, stokes));
  p.fold_whole ();
  rec::note ("## ndim 1: not recorded");
  p.fold.set_input (intensity);
  p.perform ();
  DO (p.det->polarimetry (1, p.chan, intensity));
  p.fold_whole ();
  rec::note ("## ndim 2 recorded, folded from a series that is not the detection's output");
  p.perform (); p.detect ();
  p.fold_whole ();
  rec::note ("## input ndat != output ndat");
  DO (p.det->polarimetry (2, p.chan, series (p.dmem, 4, 2, 2, NDAT + 1, Signal::Coherence)));
  rec::note ("## detection without a chain: in place, out of place, square law to Intensity");
  HIP::DetectionEngine plain (p.ctx);
  DO (plain.polarimetry (2, p.chan, p.chan));
  DO (plain.polarimetry (4, p.chan, stokes));
  DO (plain.set_output_state (Signal::Coherence));
  DO (plain.polarimetry (4, p.chan, stokes));
  intensity->set_state (Signal::Intensity);
  DO (plain.square_law (p.chan, intensity));
  p.result ();
}

static void chain_shapes (unsigned nchan, unsigned npol)
{
  for (int deferred = 0; deferred < 2; deferred++)
  {
    Pipeline p (true, deferred, nchan, npol);
    HIP::TimeSeriesEngine tse (p.ctx, p.chain);
    dsp::TimeSeries* kept = series (p.dmem, nchan, npol, 2, NDAT, Signal::Analytic);
    p.eng->get_profiles ()->set_hits_nchan (nchan);                               // (before the first prepare_output sizes hits[])
    p.block ();
    p.perform ();
    DO (tse.prepare (kept));
    DO (tse.copy_data_fpt (p.chan, 1, 3));
    DO (p.det->square_law (p.chan, kept));
    DO (p.fbe->perform_raw (0, DSPSR_AMD_RAW_GENERIC, 1.0f, p.chan, NPART, 2 * NKEEP));
    p.chan->set_zeroed_data (true);
    p.block ();
    p.result ();
  }
}
static void chain_one_channel () { chain_shapes (1, 2); }
static void chain_one_polarisation () { chain_shapes (4, 1); }

// ---- the engines that stand alone
static const unsigned SHAPES[3][2] = { {4, 2}, {1, 2}, {4, 1} };                  // (nchan, npol): zero strides must show

static void convolution ()
{
  dspsr_amd_ctx* ctx = new_ctx ();
  dsp::Memory* dmem = new HIP::DeviceMemory (ctx);
  for (int s = 0; s < 3; s++)
  {
    const unsigned nchan = SHAPES[s][0], npol = SHAPES[s][1];
    rec::note ("## nchan %u, npol %u", nchan, npol);
    dsp::TimeSeries* in = series (dmem, nchan, npol, s == 2 ? 1 : 2, 64, s == 2 ? Signal::Nyquist : Signal::Analytic);
    dsp::TimeSeries* out = series (dmem, nchan, npol, s == 2 ? 1 : 2, 64, in->get_state ());
    dsp::Response response;
    response.impulse_pos = 2; response.impulse_neg = 1; response.nchan = nchan; response.ndat = 16; response.kernel.resize (2 * nchan * 16);
    dsp::Convolution convolution;
    convolution.input = in; convolution.nsamp_fft = 16; convolution.nsamp_overlap = 3;
    HIP::ConvolutionEngine engine (ctx);
    DO (engine.set_scratch (0));
    DO (engine.prepare (&convolution));                                            // no response
    convolution.response = &response;
    DO (engine.prepare (&convolution));
    DO (engine.perform (in, out, 4));
    DO (engine.perform (in, out, 0));
    DO (engine.prepare (&convolution));                                            // a second prepare replaces the object
    DO (engine.perform (in, in, 2));
  }
}

static void matrix_setup ()
{
  dspsr_amd_ctx* ctx = new_ctx ();
  dsp::Memory* dmem = new HIP::DeviceMemory (ctx);
  dsp::TimeSeries* good = series (dmem, 1, 2, 1, 64, Signal::Nyquist);
  dsp::TimeSeries* analytic = series (dmem, 1, 2, 2, 64, Signal::Analytic);
  dsp::TimeSeries* two_chan = series (dmem, 2, 2, 1, 64, Signal::Nyquist);
  dsp::TimeSeries* one_pol = series (dmem, 1, 1, 1, 64, Signal::Nyquist);
  dsp::Response response;
  response.impulse_pos = 3; response.impulse_neg = 5; response.nchan = 4; response.ndat = 16; response.kernel.resize (8 * 4 * 16);
  dsp::Filterbank filterbank;
  filterbank.nchan_subband = 4; filterbank.freq_res = 16; filterbank.input = good;
  HIP::Chain* chain = new HIP::Chain (ctx);
  HIP::MatrixFilterbankEngine* engine = new HIP::MatrixFilterbankEngine (ctx, chain);
  DO (engine->set_fused_fold (DSPSR_AMD_FUSED_NEVER));
  DO (engine->set_max_parts (7));
  DO (engine->set_scratch (0));
  rec::note ("## no response");
  DO (engine->setup (&filterbank));
  filterbank.response = &response;
  const unsigned ndims[4] = { 2, 8, 4, 1 };
  for (int i = 0; i < 4; i++)
  {
    response.ndim = ndims[i];
    rec::note ("## ndim %u", response.ndim);
    filterbank.passband_cleared = false;
    DO (engine->setup (&filterbank));
    rec::note ("passband cleared: %d", (int) filterbank.passband_cleared);
  }
  response.ndim = 8;
  rec::note ("## ndim 8, complex input");
  filterbank.input = analytic;
  DO (engine->setup (&filterbank));
  rec::note ("## ndim 8, more than one input channel");
  filterbank.input = two_chan;
  DO (engine->setup (&filterbank));
  rec::note ("## ndim 8, npol 1");
  filterbank.input = one_pol;
  DO (engine->setup (&filterbank));
  rec::note ("## ndim 2 with the same inputs");
  response.ndim = 2;
  DO (engine->setup (&filterbank));
  filterbank.input = two_chan;
  DO (engine->setup (&filterbank));
  rec::set_response_ndim (8);
  DO (rec::note ("response_ndim %d", engine->response_ndim ()));
  rec::note ("## the base engine refuses a matrix response");
  response.ndim = 8;
  filterbank.input = good;
  HIP::FilterbankEngine base (ctx);
  DO (base.setup (&filterbank));
  rec::note ("## setup with a block pending on the chain");
  response.ndim = 8;
  chain->set_deferred (true);
  dsp::TimeSeries* out = series (dmem, 4, 2, 2, NDAT, Signal::Analytic);
  DO (engine->perform (good, out, NPART, STEP, 2 * NKEEP));
  DO (engine->setup (&filterbank));
  counters (chain);
  DO (delete engine);
}

static void scrunch ()
{
  dspsr_amd_ctx* ctx = new_ctx ();
  dsp::Memory* dmem = new HIP::DeviceMemory (ctx);
  HIP::TScrunchEngine* tscrunch = new HIP::TScrunchEngine (ctx);
  HIP::FScrunchEngine fscrunch (ctx);
  const unsigned order[4] = { 1, 2, 0, 1 };                                        // the carry grows with the second and the third shape only
  for (int s = 0; s < 4; s++)
  {
    const unsigned nchan = SHAPES[order[s]][0], npol = SHAPES[order[s]][1];
    rec::note ("## nchan %u, npol %u", nchan, npol);
    dsp::TimeSeries* in = series (dmem, nchan, npol, 2, 20, Signal::Analytic);
    dsp::TimeSeries* tout = series (dmem, nchan, npol, 2, 5, Signal::Analytic);
    DO (tscrunch->fpt_tscrunch (in, tout, 4));
    dsp::TimeSeries* fout = series (dmem, nchan > 1 ? nchan / 2 : 1, npol, 2, 20, Signal::Analytic);
    DO (fscrunch.fpt_fscrunch (in, fout, nchan > 1 ? 2 : 1));
    if (nchan == 4)
    {
      rec::note ("## nchan / sfactor == 1");
      DO (fscrunch.fpt_fscrunch (in, series (dmem, 1, npol, 2, 20, Signal::Analytic), 4));
    }
  }
  dsp::TimeSeries* in = series (dmem, 4, 2, 2, 20, Signal::Analytic);
  rec::note ("## ndim mismatch, in place, no data");
  DO (tscrunch->fpt_tscrunch (in, series (dmem, 4, 2, 1, 5, Signal::Analytic), 4));
  DO (tscrunch->fpt_tscrunch (in, in, 4));
  DO (fscrunch.fpt_fscrunch (in, in, 2));
  dsp::TimeSeries* empty = series (dmem, 4, 2, 2, 0, Signal::Analytic);
  DO (tscrunch->fpt_tscrunch (empty, in, 4));
  DO (fscrunch.fpt_fscrunch (empty, in, 2));
  DO (delete tscrunch);
  DO (delete new HIP::TScrunchEngine (ctx));                                       // no carry to free
}

static void timeseries_memory ()
{
  dspsr_amd_ctx* ctx = new_ctx ();
  HIP::DeviceMemory* dmem = new HIP::DeviceMemory (ctx);
  rec::note ("on_host %d, context %s", (int) dmem->on_host (), dmem->get_context () == ctx ? "kept" : "lost");
  void* a = 0; void* b = 0;
  DO (a = dmem->do_allocate (64));
  DO (b = dmem->do_allocate (32));
  DO (dmem->do_zero (a, 64));
  DO (dmem->do_copy (b, (char*) a + 16, 32));
  DO (dmem->do_free (a));
  DO (dmem->do_free (b));
  for (int s = 0; s < 3; s++)
  {
    const unsigned nchan = SHAPES[s][0], npol = SHAPES[s][1];
    rec::note ("## nchan %u, npol %u", nchan, npol);
    HIP::TimeSeriesEngine engine (ctx);
    dsp::TimeSeries* to = series (dmem, nchan, npol, 2, 8, Signal::Analytic);
    dsp::TimeSeries* from = series (dmem, nchan, npol, 2, 24, Signal::Analytic);
    DO (engine.prepare (to));
    DO (engine.prepare_buffer (128));
    DO (engine.copy_data_fpt (from, 16, 8));
    DO (engine.copy_data_fpt (from));
  }
  rec::note ("## the shape is the parent's: a source of another shape");
  HIP::TimeSeriesEngine engine (ctx);
  DO (engine.prepare (series (dmem, 4, 2, 2, 8, Signal::Analytic)));
  DO (engine.copy_data_fpt (series (dmem, 8, 2, 2, 8, Signal::Analytic), 3, 4));
  DO (engine.prepare (series (dmem, 1, 1, 1, 8, Signal::Nyquist)));
  DO (engine.copy_data_fpt (series (dmem, 4, 2, 2, 8, Signal::Analytic), 3, 4));
}

static void cyclic ()
{
  dspsr_amd_ctx* ctx = new_ctx ();
  dsp::Memory* dmem = new HIP::DeviceMemory (ctx);
  for (int s = 0; s < 3; s++)
  {
    const unsigned nchan = SHAPES[s][0], npol = SHAPES[s][1];
    rec::note ("## nchan %u, npol %u", nchan, npol);
    dsp::TimeSeries* in = series (dmem, nchan, npol, 2, 12, Signal::Analytic);
    dsp::CyclicFold fold;
    HIP::CyclicFoldEngine* engine = new HIP::CyclicFoldEngine (ctx);
    fold.set_input (in); fold.set_engine (engine); fold.set_nbin (4);
    fold.set_nlag (3); fold.set_mover (1); fold.set_npol (npol == 2 ? 4 : 1);
    DO (fold.prepare ());
    DO (fold.prepare_output ());
    DO (fold.fold (0.25, 3e-6, 2, 6));                                             // set_nbin, set_ndat, set_bin per sample, fold
    rec::note ("lagdata size %llu", (unsigned long long) engine->get_lagdata_size ());
    DO (fold.get_result ());
    DO (fold.get_result ());                                                       // synchronized: nothing
    DO (fold.fold (0.5, 3e-6, 0, 12));
    DO (fold.reset ());
    DO (fold.get_result ());
    DO (delete engine);
  }
  rec::note ("## synch before set_ndat, real input, host input");
  dsp::CyclicFold fold;
  HIP::CyclicFoldEngine* engine = new HIP::CyclicFoldEngine (ctx);
  fold.set_input (series (dmem, 2, 2, 2, 12, Signal::Analytic)); fold.set_engine (engine); fold.set_nbin (4);
  fold.set_nlag (3); fold.set_npol (2);
  DO (fold.prepare ());
  DO (fold.prepare_output ());
  DO (engine->fold ());
  DO (engine->synch (fold.get_output ()));
  fold.set_input (series (dmem, 2, 2, 1, 12, Signal::Nyquist));
  DO (engine->set_ndat (6, 0));
  fold.set_input (series (0, 2, 2, 2, 12, Signal::Analytic));
  DO (engine->set_ndat (6, 0));
  DO (engine->fold ());
}

static void spectral_kurtosis ()
{
  dspsr_amd_ctx* ctx = new_ctx ();
  dsp::Memory* dmem = new HIP::DeviceMemory (ctx);
  dsp::BitSeries mask;
  rec::set_sk_npart (2);
  for (int s = 0; s < 3; s++)
  {
    const unsigned nchan = SHAPES[s][0], npol = SHAPES[s][1];
    rec::note ("## nchan %u, npol %u", nchan, npol);
    dsp::TimeSeries* in = series (dmem, nchan, npol, 2, 16, Signal::Analytic);
    dsp::TimeSeries* out = series (dmem, nchan, npol, 2, 16, Signal::Analytic);
    dsp::TimeSeries estimates, estimates_tscr;
    HIP::SpectralKurtosisEngine* engine = new HIP::SpectralKurtosisEngine (ctx, 4);
    DO (engine->setup ());
    DO (engine->mask (&mask, in, out, 8));                                         // before compute: the shape is not known yet
    DO (engine->compute (in, &estimates, &estimates_tscr, 8));
    DO (engine->reset_mask (&mask));
    DO (engine->detect_tscr (&estimates, &estimates_tscr, &mask, 1.5f, 0.5f));
    DO (engine->detect_ft (&estimates, &mask, 1.25f, 0.75f));
    DO (engine->detect_fscr (&estimates, &mask, 0.9f, 1.1f, 0, nchan));            // chan_end == nchan
    DO (engine->detect_fscr (&estimates, &mask, 0.9f, 1.1f, 1, 3));
    DO (rec::note ("count_mask %d", engine->count_mask (&mask)));
    DO (engine->get_estimates (&estimates));
    DO (engine->get_zapmask (&mask));
    DO (engine->mask (&mask, in, out, 8));
    DO (engine->insertsk (in, out, 8));
    DO (engine->set_channel_range (1, 0));
    DO (engine->compute (in, &estimates, &estimates_tscr, 8));
    DO (engine->set_channel_range (0, nchan));
    DO (engine->compute (in, &estimates, &estimates_tscr, 4));
    rec::note ("handle %s", engine->get_handle () ? "kept" : "null");
    DO (delete engine);
  }
  rec::note ("## host memory, real input");
  HIP::SpectralKurtosisEngine engine (ctx);
  dsp::TimeSeries* device = series (dmem, 2, 2, 2, 16, Signal::Analytic);
  dsp::TimeSeries* host = series (0, 2, 2, 2, 16, Signal::Analytic);
  DO (engine.compute (host, 0, 0, 8));
  DO (engine.compute (series (dmem, 2, 2, 1, 16, Signal::Nyquist), 0, 0, 8));
  DO (engine.mask (&mask, host, device, 8));
  DO (engine.mask (&mask, device, host, 8));
}

// ---- every status the library can return, through every copy of the status-to-Error mapping
static void failures (int code)
{
  Pipeline p (true, false);
  HIP::TimeSeriesEngine tse (p.ctx);
  tse.prepare (p.chan);
  rec::fail ("dspsr_amd_filterbank_create", code); DO (p.fbe->setup (&p.filterbank));
  rec::fail ("dspsr_amd_filterbank_set_kernel", code); DO (p.fbe->setup (&p.filterbank));
  rec::fail ("dspsr_amd_filterbank_perform", code); p.perform ();
  rec::fail ("dspsr_amd_filterbank_perform_raw", code); DO (p.fbe->perform_raw (0, 0, 1.0f, p.chan, NPART, 2 * NKEEP));
  rec::fail ("dspsr_amd_stream_sync", code); DO (p.fbe->finish ());
  rec::fail ("dspsr_amd_detect_polarimetry", code); p.detect ();
  rec::fail ("dspsr_amd_detect_square_law", code); DO (p.det->square_law (p.chan, p.chan));
  rec::fail ("dspsr_amd_copy_fpt", code); DO (tse.copy_data_fpt (p.chan, 0, 4));
  rec::fail ("dspsr_amd_malloc", code); DO (p.dmem->do_allocate (16));
  rec::fail ("dspsr_amd_free", code); DO (p.dmem->do_free (0));
  rec::fail ("dspsr_amd_zero", code); DO (p.dmem->do_zero (0, 0));
  rec::fail ("dspsr_amd_copy", code); DO (p.dmem->do_copy (0, 0, 0));
  dsp::BitSeries bits;
  rec::fail ("dspsr_amd_copy", code); DO (HIP::transfer_bitseries (p.ctx, &bits, &bits, p.fbe, 0, 1.0f));
  DO (p.fold.prepare_output ());
  rec::fail ("dspsr_amd_fold_set_nbin", code); DO (p.eng->set_nbin (NBIN));
  rec::fail ("dspsr_amd_fold_set_ndat", code); DO (p.eng->set_ndat (NDAT, 0));
  rec::fail ("dspsr_amd_fold_set_bin", code); DO (p.eng->set_bin (0, 0.5, 0.25));
  rec::fail ("dspsr_amd_fold_set_bins", code); DO (p.eng->set_bins (0.25, 0.125, NDAT, 0));
  rec::fail ("dspsr_amd_fold_bind_profile", code); DO (p.eng->fold ());
  rec::fail ("dspsr_amd_fold_fold", code); DO (p.eng->fold ());
  rec::fail ("dspsr_amd_copy", code); DO (p.fold.get_result ());
  rec::fail ("dspsr_amd_stream_sync", code); DO (p.fold.get_result ());
  p.chan->set_zeroed_data (true);
  p.eng->get_profiles ()->set_hits_nchan (4);
  rec::fail ("dspsr_amd_malloc", code); DO (p.eng->fold ());
  rec::fail ("dspsr_amd_zero", code); DO (p.eng->fold ());
  rec::fail ("dspsr_amd_fold_fold_zeroed", code); DO (p.eng->fold ());
  rec::fail ("dspsr_amd_zero", code); DO (p.eng->zero ());
  rec::fail ("dspsr_amd_fold_create", code); DO (new HIP::FoldEngine (p.ctx));
  p.chain->set_deferred (true);
  p.chan->set_zeroed_data (false);
  p.perform (); p.detect ();
  rec::fail ("dspsr_amd_filterbank_perform_fold", code); p.fold_whole ();
  p.counters_if ();

  dsp::Convolution convolution;
  convolution.input = p.in; convolution.response = &p.response; convolution.nsamp_fft = 16; convolution.nsamp_overlap = 8;
  HIP::ConvolutionEngine ce (p.ctx);
  rec::fail ("dspsr_amd_filterbank_create", code); DO (ce.prepare (&convolution));
  rec::fail ("dspsr_amd_filterbank_set_kernel", code); DO (ce.prepare (&convolution));
  rec::fail ("dspsr_amd_filterbank_perform", code); DO (ce.perform (p.in, p.in, 1));

  p.response.ndim = 8;
  HIP::MatrixFilterbankEngine me (p.ctx);
  rec::fail ("dspsr_amd_filterbank_create", code); DO (me.setup (&p.filterbank));
  rec::fail ("dspsr_amd_filterbank_set_response_matrix", code); DO (me.setup (&p.filterbank));

  HIP::TScrunchEngine ts (p.ctx);
  HIP::FScrunchEngine fs (p.ctx);
  dsp::TimeSeries* small = series (p.dmem, 4, 2, 2, 6, Signal::Analytic);
  rec::fail ("dspsr_amd_malloc", code); DO (ts.fpt_tscrunch (p.chan, small, 4));
  rec::fail ("dspsr_amd_tscrunch_fpt", code); DO (ts.fpt_tscrunch (p.chan, small, 4));
  rec::fail ("dspsr_amd_fscrunch_fpt", code); DO (fs.fpt_fscrunch (p.chan, small, 2));

  dsp::CyclicFold cfold;
  rec::fail ("dspsr_amd_cyclic_fold_create", code); DO (new HIP::CyclicFoldEngine (p.ctx));
  HIP::CyclicFoldEngine* cyc = new HIP::CyclicFoldEngine (p.ctx);
  cfold.set_input (p.chan); cfold.set_engine (cyc); cfold.set_nbin (4); cfold.set_nlag (3); cfold.set_npol (2);
  cfold.prepare (); cfold.prepare_output ();
  rec::fail ("dspsr_amd_cyclic_fold_set_shape", code); DO (cyc->set_ndat (6, 0));
  rec::fail ("dspsr_amd_cyclic_fold_set_ndat", code); DO (cyc->set_ndat (6, 0));
  DO (cyc->set_ndat (6, 0));
  rec::fail ("dspsr_amd_cyclic_fold_set_bin", code); DO (cyc->set_bin (0, 0.5, 0.25));
  rec::fail ("dspsr_amd_cyclic_fold_fold", code); DO (cyc->fold ());
  rec::fail ("dspsr_amd_cyclic_fold_zero", code); DO (cyc->zero ());
  DO (cyc->fold ());
  rec::fail ("dspsr_amd_cyclic_fold_synch_lags", code); DO (cyc->synch (cfold.get_output ()));

  dsp::BitSeries mask;
  rec::fail ("dspsr_amd_sk_create", code); DO (new HIP::SpectralKurtosisEngine (p.ctx));
  HIP::SpectralKurtosisEngine sk (p.ctx);
  rec::fail ("dspsr_amd_sk_set_shape", code); DO (sk.compute (p.chan, 0, 0, 8));
  rec::fail ("dspsr_amd_sk_set_options", code); DO (sk.compute (p.chan, 0, 0, 8));
  rec::fail ("dspsr_amd_sk_compute", code); DO (sk.compute (p.chan, 0, 0, 8));
  rec::fail ("dspsr_amd_sk_reset_mask", code); DO (sk.reset_mask (&mask));
  rec::fail ("dspsr_amd_sk_detect_skfb", code); DO (sk.detect_ft (0, &mask, 1.25f, 0.75f));
  rec::fail ("dspsr_amd_sk_set_options", code); DO (sk.detect_fscr (0, &mask, 0, 0, 0, 4));
  rec::fail ("dspsr_amd_sk_detect_fscr", code); DO (sk.detect_fscr (0, &mask, 0, 0, 0, 4));
  rec::fail ("dspsr_amd_sk_detect_tscr", code); DO (sk.detect_tscr (0, 0, &mask, 1.5f, 0.5f));
  rec::fail ("dspsr_amd_copy", code); DO (sk.count_mask (&mask));
  rec::fail ("dspsr_amd_copy", code); DO (sk.get_estimates (0));
  rec::fail ("dspsr_amd_copy", code); DO (sk.get_zapmask (&mask));
  rec::fail ("dspsr_amd_sk_mask", code); DO (sk.mask (&mask, p.chan, p.chan, 8));
}
static void failures_einval () { failures (DSPSR_AMD_EINVAL); }
static void failures_ehip () { failures (DSPSR_AMD_EHIP); }
static void failures_enomem () { failures (DSPSR_AMD_ENOMEM); }
static void failures_estate () { failures (DSPSR_AMD_ESTATE); }

static void no_context ()
{
  dsp::TimeSeries* in = series (0, 1, 2, 1, 64, Signal::Nyquist);
  dsp::Filterbank filterbank;
  filterbank.nchan_subband = 4; filterbank.freq_res = 16; filterbank.input = in;
  HIP::FilterbankEngine fbe (0);
  DO (fbe.setup (&filterbank));
  DO (new HIP::FoldEngine (0));
  DO (new HIP::CyclicFoldEngine (0));
  DO (new HIP::SpectralKurtosisEngine (0));
}

static const struct { const char* name; void (*run) (); } scenarios[] = {
  { "chain_none", chain_none }, { "chain_eager", chain_eager }, { "chain_deferred_float", chain_deferred_float },
  { "chain_deferred_raw", chain_deferred_raw }, { "chain_finish_each", chain_finish_each }, { "chain_pieces", chain_pieces },
  { "chain_two_folds", chain_two_folds }, { "chain_zeroed", chain_zeroed }, { "chain_unfolded", chain_unfolded },
  { "chain_refused_readers", chain_refused_readers }, { "chain_pending", chain_pending },
  { "chain_detected_shapes", chain_detected_shapes }, { "chain_one_channel", chain_one_channel },
  { "chain_one_polarisation", chain_one_polarisation }, { "convolution", convolution }, { "matrix_setup", matrix_setup },
  { "scrunch", scrunch }, { "timeseries_memory", timeseries_memory }, { "cyclic", cyclic },
  { "spectral_kurtosis", spectral_kurtosis }, { "failures_einval", failures_einval }, { "failures_ehip", failures_ehip },
  { "failures_enomem", failures_enomem }, { "failures_estate", failures_estate }, { "no_context", no_context },
};

//! a library message is data, never a format: one holding a conversion must arrive as it is, from every engine family
static int messages ()
{
  const char* text = "row %d of 100%% is bad";
  int bad = 0;
  rec::reset ();
  dspsr_amd_ctx* ctx = new_ctx ();
  std::string got[3];
  rec::fail ("dspsr_amd_stream_sync", DSPSR_AMD_EHIP, text);
  try { HIP::FilterbankEngine (ctx).finish (); } catch (Error& e) { got[0] = e.message; }
  HIP::CyclicFoldEngine cyc (ctx);
  rec::fail ("dspsr_amd_cyclic_fold_set_bin", DSPSR_AMD_EHIP, text);
  try { cyc.set_bin (0, 0, 0); } catch (Error& e) { got[1] = e.message; }
  HIP::SpectralKurtosisEngine sk (ctx);
  rec::fail ("dspsr_amd_sk_reset_mask", DSPSR_AMD_EHIP, text);
  try { sk.reset_mask (0); } catch (Error& e) { got[2] = e.message; }
  const char* method[3] = { "HIP::FilterbankEngine::finish", "HIP::CyclicFoldEngine::set_bin", "HIP::SpectralKurtosisEngine::reset_mask" };
  for (int i = 0; i < 3; i++)
  {
    const std::string want = std::string (method[i]) + ": " + text;
    if (got[i] != want) { printf ("FAILED: \"%s\" arrived as \"%s\"\n", want.c_str (), got[i].c_str ()); bad = 1; }
  }
  if (!bad) printf ("messages ok\n");
  return bad;
}

int main (int argc, char** argv)
{
  if (argc == 2 && !strcmp (argv[1], "--messages")) return messages ();
  if (argc != 2) { fprintf (stderr, "usage: %s DIR | --messages\n", argv[0]); return 2; }
  for (size_t i = 0; i < sizeof scenarios / sizeof scenarios[0]; i++)
  {
    rec::reset ();
    try { scenarios[i].run (); }
    catch (Error& e) { rec::note ("the scenario ended with:"); note_error (e); }
    const std::string path = std::string (argv[1]) + "/" + scenarios[i].name + ".txt";
    FILE* fp = fopen (path.c_str (), "w");
    if (!fp) { fprintf (stderr, "cannot write %s\n", path.c_str ()); return 2; }
    fputs (rec::text ().c_str (), fp);
    fclose (fp);
  }
  return 0;
}
