// Drives HIP::MatrixFilterbankEngine (dspsr_amd/host/dspsr_amd_matrix_engine.h) against the miniature dsp classes of
// tests/host_mock (its dsp::Response has get_ndim ()).
// Without a device: the reference's two errors (Filterbank.C:199-205) and the base engine's refusal of a matrix response are
// thrown before any library call; exit code 77.  On a GPU: an ndim 8 response reaches dspsr_amd_filterbank_set_response_matrix,
// an ndim 2 response dspsr_amd_filterbank_set_kernel, each bit-identical to the C-ABI driven directly.
// Built and run by tests/test_host_adaptor_matrix.py.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "dspsr_amd_matrix_engine.h"

#define REQUIRE(cond, what) do { if (!(cond)) { printf ("FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); return 1; } } while (0)

static unsigned lcg = 12345u;
static float rnd () { lcg = lcg * 1664525u + 1013904223u; return (float) ((int) (lcg >> 8) % 2001 - 1000) / 1000.0f; }

static const unsigned C = 8, M = 64, POS = 5, NEG = 7, NKEEP = M - POS - NEG, NPART = 3;
static const uint64_t N = uint64_t (C) * M, STEP = 2 * N - 2 * (POS + NEG) * C;

static void shape_input (dsp::TimeSeries& t, unsigned nchan, unsigned npol)
{
  t.set_nchan (nchan); t.set_npol (npol); t.set_ndim (1); t.set_state (Signal::Nyquist); t.set_rate (1e6);
}

static void make_response (dsp::Response& r, unsigned ndim)
{
  r.impulse_pos = POS; r.impulse_neg = NEG; r.nchan = C; r.ndat = M; r.ndim = ndim;
  r.kernel.resize (N * ndim);
  for (uint64_t k = 0; k < N * ndim; k++) r.kernel[k] = rnd ();
}

template <class E> static std::string thrown_by (E& engine, dsp::Filterbank* fbk)
{
  try { engine.setup (fbk); }
  catch (Error& e) { return e.message; }
  return "";
}

static int run (dspsr_amd_ctx* ctx, dsp::Memory* dmem, const dsp::TimeSeries& in_d, unsigned ndim)
{
  dsp::Response resp;
  make_response (resp, ndim);
  dsp::Filterbank fbk;
  fbk.nchan_subband = C; fbk.freq_res = M; fbk.input = &in_d; fbk.response = &resp;
  HIP::MatrixFilterbankEngine fbe (ctx);
  fbe.setup (&fbk);
  REQUIRE (fbk.passband_cleared, "setup must null the passband (FilterbankCUDA.cu:78)");
  REQUIRE (fbe.response_ndim () == (int) ndim, "the library object must hold the response's ndim");
  dsp::TimeSeries out_d, out2_d, out_h, out2_h;
  out_d.set_nchan (C); out_d.set_npol (2); out_d.set_ndim (2); out_d.set_state (Signal::Analytic); out_d.set_rate (1e6 / (2 * C));
  out_d.set_memory (dmem); out_d.resize (NPART * NKEEP);
  out2_d.set_memory (dmem); out2_d.internal_match (&out_d);
  out_h.internal_match (&out_d); out2_h.internal_match (&out_d);
  fbe.perform (&in_d, &out_d, NPART, STEP, 2 * NKEEP);
  fbe.finish ();
  {  // the same through the bare C-ABI
    dspsr_amd_filterbank_config cfg = {C, M, POS, NEG, 1, 2, 1, 0, 0, DSPSR_AMD_FUSED_AUTO};
    dspsr_amd_filterbank* fb = 0;
    HIP::check (ctx, dspsr_amd_filterbank_create (ctx, &cfg, &fb), "create");
    if (ndim == 8) HIP::check (ctx, dspsr_amd_filterbank_set_response_matrix (fb, &resp.kernel[0], N), "set_response_matrix");
    else HIP::check (ctx, dspsr_amd_filterbank_set_kernel (fb, &resp.kernel[0], N), "set_kernel");
    HIP::check (ctx, dspsr_amd_filterbank_perform (fb, in_d.get_datptr (0, 0), 0, in_d.get_datptr (0, 1) - in_d.get_datptr (0, 0),
             out2_d.get_datptr (0, 0), out2_d.get_datptr (1, 0) - out2_d.get_datptr (0, 0),
             out2_d.get_datptr (0, 1) - out2_d.get_datptr (0, 0), NPART, STEP, 2 * NKEEP), "perform");
    HIP::check (ctx, dspsr_amd_stream_sync (ctx), "sync");
    dspsr_amd_filterbank_destroy (fb);
  }
  HIP::check (ctx, dspsr_amd_copy (ctx, out_h.internal_get_buffer (), out_d.internal_get_buffer (), out_d.internal_get_size (), DSPSR_AMD_D2H), "d2h");
  HIP::check (ctx, dspsr_amd_copy (ctx, out2_h.internal_get_buffer (), out2_d.internal_get_buffer (), out2_d.internal_get_size (), DSPSR_AMD_D2H), "d2h");
  HIP::check (ctx, dspsr_amd_stream_sync (ctx), "d2h");
  double power = 0;
  for (unsigned c = 0; c < C; c++) for (unsigned p = 0; p < 2; p++) for (unsigned i = 0; i < 2 * NPART * NKEEP; i++) {
    REQUIRE (out_h.get_datptr (c, p)[i] == out2_h.get_datptr (c, p)[i], "MatrixFilterbankEngine::perform differs from the C-ABI");
    power += double (out_h.get_datptr (c, p)[i]) * out_h.get_datptr (c, p)[i];
  }
  REQUIRE (power > 0, "filterbank output is all zero");
  printf ("ndim %u: %s entry point, bit-identical to the C-ABI\n", ndim, ndim == 8 ? "matrix" : "scalar");
  return 0;
}

int main ()
{
  try {
    // ---- host: refusals that come before any library call (a null context is never touched)
    dsp::Response r8;
    make_response (r8, 8);
    dsp::TimeSeries two_chan, one_pol, good;
    shape_input (two_chan, 2, 2); shape_input (one_pol, 1, 1); shape_input (good, 1, 2);
    dsp::Filterbank fbk;
    fbk.nchan_subband = C; fbk.freq_res = M; fbk.response = &r8;
    HIP::MatrixFilterbankEngine me (0);
    fbk.input = &two_chan;
    REQUIRE (thrown_by (me, &fbk).find ("matrix convolution untested for > one input channel") != std::string::npos, "Filterbank.C:199-201");
    fbk.input = &one_pol;
    REQUIRE (thrown_by (me, &fbk).find ("matrix convolution and input.npol != 2") != std::string::npos, "Filterbank.C:203-205");
    HIP::FilterbankEngine base (0);
    fbk.input = &good;
    REQUIRE (thrown_by (base, &fbk).find ("MatrixFilterbankEngine") != std::string::npos, "the base engine must refuse a matrix response");
    printf ("host engine ok\n");

    dspsr_amd_ctx* ctx = 0;
    if (dspsr_amd_ctx_create (0, DSPSR_AMD_NEW_STREAM, &ctx) != DSPSR_AMD_OK) { printf ("no HIP device\n"); return 77; }
    dsp::Memory* dmem = new HIP::DeviceMemory (ctx);
    dsp::TimeSeries in_h, in_d;
    shape_input (in_h, 1, 2);
    in_h.resize (NPART * STEP + 2 * (POS + NEG) * C);
    in_d.set_memory (dmem); in_d.internal_match (&in_h);
    for (unsigned p = 0; p < 2; p++) for (uint64_t i = 0; i < in_h.get_ndat (); i++) in_h.get_datptr (0, p)[i] = rnd ();
    HIP::check (ctx, dspsr_amd_copy (ctx, in_d.internal_get_buffer (), in_h.internal_get_buffer (), in_h.internal_get_size (), DSPSR_AMD_H2D), "h2d");
    HIP::check (ctx, dspsr_amd_stream_sync (ctx), "h2d");
    if (run (ctx, dmem, in_d, 8) || run (ctx, dmem, in_d, 2)) return 1;
    // a geometry the library refuses surfaces as an Error carrying its message
    {
      dsp::Response r;
      make_response (r, 8);
      r.nchan = 1; r.ndat = M;
      dsp::Filterbank f1;
      f1.nchan_subband = 1; f1.freq_res = M; f1.input = &in_d; f1.response = &r;
      HIP::MatrixFilterbankEngine e1 (ctx);
      REQUIRE (thrown_by (e1, &f1).find ("nchan_subband") != std::string::npos, "nchan_subband = 1 must be refused by name");
    }
    printf ("matrix adaptor driver ok\n");
    dspsr_amd_ctx_destroy (ctx);
    return 0;
  }
  catch (Error& e) { printf ("FAILED: Error: %s\n", e.message.c_str ()); return 1; }
}
