// A recording stand-in for libdspsr_amd: every dspsr_amd_* function that the adaptor headers of dspsr_amd/host call, in plain
// C++ without HIP.  The memory calls act on host memory; every call appends one line to a log and returns DSPSR_AMD_OK or the
// status armed with rec::fail; the few calls whose results the adaptors read return the values set through tests/capi_recorder.h.
// In the log an object is "<kind><creation ordinal>", a pointer "b<allocation ordinal>+<byte offset>" when it lies inside a live
// allocation of dspsr_amd_malloc (or a device array of an object), "host" otherwise and "null"; floating point is printed with %a.
// tests/adaptor_trace_driver.cpp drives the adaptors over it; tests/test_adaptor_trace_host.py compares the logs with
// tests/golden/adaptor_trace/.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dspsr_amd.h"
#include "capi_recorder.h"

struct dspsr_amd_ctx { int ord; std::string error; };
struct dspsr_amd_filterbank { int ord; dspsr_amd_ctx* ctx; };
struct dspsr_amd_fold { int ord; dspsr_amd_ctx* ctx; uint32_t nbin; };
struct dspsr_amd_cyclic_fold { int ord; dspsr_amd_ctx* ctx; };
struct dspsr_amd_sk { int ord; dspsr_amd_ctx* ctx; void* estimates; void* zapmask; };

namespace
{
  struct Buffer { int ord; char* base; size_t size; bool live; };
  std::vector<Buffer> buffers;
  std::string log_text;
  int nctx, nfb, nfold, ncyclic, nsk;
  std::string fail_function, fail_message;
  int fail_code;
  uint64_t step_value, folded_value, sk_npart_value;
  uint32_t hits_value;
  int response_ndim_value;

  void* allocate (size_t nbytes)
  {
    Buffer b = { (int) buffers.size (), (char*) calloc (nbytes ? nbytes : 1, 1), nbytes, true };
    buffers.push_back (b);
    return b.base;
  }
  bool release (void* p)
  {
    for (size_t i = 0; i < buffers.size (); i++)
      if (buffers[i].live && buffers[i].base == p) { buffers[i].live = false; free (p); return true; }
    return false;
  }

  //! a pointer as the log shows it
  std::string pointer_text (const void* q)
  {
    if (!q) return "null";
    for (size_t k = 0; k < buffers.size (); k++)
    {
      const Buffer& b = buffers[k];
      if (b.live && (const char*) q >= b.base && (const char*) q < b.base + (b.size ? b.size : 1))
        return "b" + std::to_string (b.ord) + "+" + std::to_string ((const char*) q - b.base);
    }
    return "host";
  }

  //! one line of the log: name (arguments) -> result
  struct Call
  {
    std::string line;
    const char* name;
    bool first;
    Call (const char* _name) : line (_name), name (_name), first (true) { line += " ("; }
    Call& text (const std::string& t) { if (!first) line += ", "; first = false; line += t; return *this; }
    Call& fmt (const char* f, ...)
    {
      char buf[512];
      va_list ap; va_start (ap, f); vsnprintf (buf, sizeof buf, f, ap); va_end (ap);
      return text (buf);
    }
    Call& u (uint64_t v) { return fmt ("%llu", (unsigned long long) v); }
    Call& i (int64_t v) { return fmt ("%lld", (long long) v); }
    Call& f (double v) { return fmt ("%a", v); }
    Call& p (const void* q) { return text (pointer_text (q)); }
    Call& obj (const char* kind, const void* o, int ord) { return o ? fmt ("%s%d", kind, ord) : text ("null"); }
    Call& c (const dspsr_amd_ctx* o) { return obj ("ctx", o, o ? o->ord : 0); }
    Call& o (const dspsr_amd_filterbank* o) { return obj ("fb", o, o ? o->ord : 0); }
    Call& o (const dspsr_amd_fold* o) { return obj ("fold", o, o ? o->ord : 0); }
    Call& o (const dspsr_amd_cyclic_fold* o) { return obj ("cyclic", o, o ? o->ord : 0); }
    Call& o (const dspsr_amd_sk* o) { return obj ("sk", o, o ? o->ord : 0); }

    void end (const std::string& result = "") { log_text += line + ")" + (result.empty () ? "" : " -> " + result) + "\n"; }
    //! the status of this call: the armed failure if it names this function (its message goes to `ctx`), else `ok`
    int status (dspsr_amd_ctx* ctx, int ok = DSPSR_AMD_OK)
    {
      int code = ok;
      if (fail_function == name)
      {
        code = fail_code;
        char buf[128];
        snprintf (buf, sizeof buf, "%s: scripted failure (%d)", name, code);
        if (ctx) ctx->error = fail_message.empty () ? std::string (buf) : fail_message;
        fail_function.clear ();
      }
      char buf[32];
      snprintf (buf, sizeof buf, "%d", code);
      end (buf);
      return code;
    }
  };
}

namespace rec
{
  void reset ()
  {
    for (size_t i = 0; i < buffers.size (); i++) buffers[i].live = false;      // (what a scenario left allocated is leaked)
    buffers.clear ();
    log_text.clear ();
    nctx = nfb = nfold = ncyclic = nsk = 0;
    fail_function.clear (); fail_message.clear (); fail_code = 0;
    step_value = 0; folded_value = 0; hits_value = 0; sk_npart_value = 0; response_ndim_value = 0;
  }
  void note (const char* fmt, ...)
  {
    char buf[1200];
    va_list ap; va_start (ap, fmt); vsnprintf (buf, sizeof buf, fmt, ap); va_end (ap);
    log_text += buf; log_text += "\n";
  }
  void fail (const char* function, int code, const char* message)
  { fail_function = function; fail_code = code; fail_message = message ? message : ""; }
  const std::string& text () { return log_text; }
  void set_step (uint64_t v) { step_value = v; }
  void set_fold (uint32_t hits, uint64_t folded) { hits_value = hits; folded_value = folded; }
  void set_sk_npart (uint64_t v) { sk_npart_value = v; }
  void set_response_ndim (int v) { response_ndim_value = v; }
}

extern "C" {

// ---- context and memory
int dspsr_amd_ctx_create (int device, void* stream, dspsr_amd_ctx** ctx)
{
  Call call ("dspsr_amd_ctx_create");
  call.i (device).text (stream ? "stream" : "null");
  const int code = call.status (0);
  if (code == DSPSR_AMD_OK) { *ctx = new dspsr_amd_ctx; (*ctx)->ord = nctx ++; }
  return code;
}
void dspsr_amd_ctx_destroy (dspsr_amd_ctx* ctx) { Call ("dspsr_amd_ctx_destroy").c (ctx).end (); }
// (not logged: the adaptors call it only to word an Error, which the driver logs)
const char* dspsr_amd_last_error (const dspsr_amd_ctx* ctx) { return ctx ? ctx->error.c_str () : "null context"; }
int dspsr_amd_stream_sync (dspsr_amd_ctx* ctx) { return Call ("dspsr_amd_stream_sync").c (ctx).status (ctx); }

int dspsr_amd_malloc (dspsr_amd_ctx* ctx, size_t nbytes, void** ptr)
{
  Call call ("dspsr_amd_malloc");
  call.c (ctx).u (nbytes);
  const int code = call.status (ctx);
  if (code == DSPSR_AMD_OK) { *ptr = allocate (nbytes); rec::note ("  = b%d", buffers.back ().ord); }
  return code;
}
int dspsr_amd_free (dspsr_amd_ctx* ctx, void* ptr)
{
  Call call ("dspsr_amd_free");
  call.c (ctx).p (ptr);
  const int code = call.status (ctx);
  if (code == DSPSR_AMD_OK && ptr && !release (ptr)) rec::note ("  (not a live allocation)");
  return code;
}
int dspsr_amd_zero (dspsr_amd_ctx* ctx, void* ptr, size_t nbytes)
{
  Call call ("dspsr_amd_zero");
  call.c (ctx).p (ptr).u (nbytes);
  const int code = call.status (ctx);
  if (code == DSPSR_AMD_OK && ptr) memset (ptr, 0, nbytes);
  return code;
}
int dspsr_amd_copy (dspsr_amd_ctx* ctx, void* dst, const void* src, size_t nbytes, int kind)
{
  Call call ("dspsr_amd_copy");
  call.c (ctx).p (dst).p (src).u (nbytes).text (kind == DSPSR_AMD_H2D ? "H2D" : kind == DSPSR_AMD_D2H ? "D2H" : kind == DSPSR_AMD_D2D ? "D2D" : "?");
  const int code = call.status (ctx);
  if (code == DSPSR_AMD_OK && dst && src) memmove (dst, src, nbytes);
  return code;
}
int dspsr_amd_copy_fpt (dspsr_amd_ctx* ctx, float* to, uint64_t tcs, uint64_t tps, const float* from, uint64_t fcs, uint64_t fps,
                        uint32_t nchan, uint32_t npol, uint64_t nfloat)
{
  Call call ("dspsr_amd_copy_fpt");
  call.c (ctx).p (to).u (tcs).u (tps).p (from).u (fcs).u (fps).u (nchan).u (npol).u (nfloat);
  const int code = call.status (ctx);
  if (code == DSPSR_AMD_OK)
    for (uint32_t c = 0; c < nchan; c++)
      for (uint32_t p = 0; p < npol; p++)
        memmove (to + c * tcs + p * tps, from + c * fcs + p * fps, nfloat * sizeof (float));
  return code;
}

// ---- filterbank
int dspsr_amd_filterbank_create (dspsr_amd_ctx* ctx, const dspsr_amd_filterbank_config* cfg, dspsr_amd_filterbank** fb)
{
  Call call ("dspsr_amd_filterbank_create");
  call.c (ctx).fmt ("{nchan_subband %u, freq_res %u, nfilt_pos %u, nfilt_neg %u, input_nchan %u, npol %u, real_input %u, max_parts %u, "
                    "force_four_pass %u, fused_fold %u, split_in_inverse %u}", cfg->nchan_subband, cfg->freq_res, cfg->nfilt_pos,
                    cfg->nfilt_neg, cfg->input_nchan, cfg->npol, cfg->real_input, cfg->max_parts, cfg->force_four_pass, cfg->fused_fold,
                    cfg->split_in_inverse);
  const int code = call.status (ctx, ctx ? DSPSR_AMD_OK : DSPSR_AMD_EINVAL);
  if (code == DSPSR_AMD_OK) { *fb = new dspsr_amd_filterbank; (*fb)->ord = nfb ++; (*fb)->ctx = ctx; rec::note ("  = fb%d", (*fb)->ord); }
  return code;
}
void dspsr_amd_filterbank_destroy (dspsr_amd_filterbank* fb) { Call ("dspsr_amd_filterbank_destroy").o (fb).end (); }
int dspsr_amd_filterbank_set_kernel (dspsr_amd_filterbank* fb, const float* kernel, uint64_t ncomplex)
{ return Call ("dspsr_amd_filterbank_set_kernel").o (fb).p (kernel).u (ncomplex).status (fb ? fb->ctx : 0); }
int dspsr_amd_filterbank_set_response_matrix (dspsr_amd_filterbank* fb, const float* response, uint64_t nmatrix)
{ return Call ("dspsr_amd_filterbank_set_response_matrix").o (fb).p (response).u (nmatrix).status (fb ? fb->ctx : 0); }
int dspsr_amd_filterbank_response_ndim (const dspsr_amd_filterbank* fb)
{
  Call call ("dspsr_amd_filterbank_response_ndim");
  call.o (fb).end (std::to_string (response_ndim_value));
  return response_ndim_value;
}
int dspsr_amd_filterbank_sizes (const dspsr_amd_filterbank* fb, uint64_t* nsamp_fft, uint64_t* nsamp_overlap, uint64_t* nsamp_step,
                                uint32_t* nkeep)
{
  Call call ("dspsr_amd_filterbank_sizes");
  call.o (fb).text (nsamp_fft ? "fft" : "null").text (nsamp_overlap ? "overlap" : "null").text (nsamp_step ? "step" : "null")
      .text (nkeep ? "nkeep" : "null");
  if (nsamp_fft) *nsamp_fft = 0;
  if (nsamp_overlap) *nsamp_overlap = 0;
  if (nsamp_step) *nsamp_step = step_value;
  if (nkeep) *nkeep = 0;
  return call.status (fb ? fb->ctx : 0);
}
int dspsr_amd_filterbank_perform (dspsr_amd_filterbank* fb, const float* in, uint64_t ics, uint64_t ips, float* out, uint64_t ocs,
                                  uint64_t ops, uint64_t npart, uint64_t in_step, uint64_t out_step)
{
  return Call ("dspsr_amd_filterbank_perform").o (fb).p (in).u (ics).u (ips).p (out).u (ocs).u (ops).u (npart).u (in_step).u (out_step)
         .status (fb ? fb->ctx : 0);
}
int dspsr_amd_filterbank_perform_raw (dspsr_amd_filterbank* fb, const int8_t* raw, int layout, float scale, float* out, uint64_t ocs,
                                      uint64_t ops, uint64_t npart, uint64_t out_step)
{
  return Call ("dspsr_amd_filterbank_perform_raw").o (fb).p (raw).i (layout).f (scale).p (out).u (ocs).u (ops).u (npart).u (out_step)
         .status (fb ? fb->ctx : 0);
}
int dspsr_amd_filterbank_perform_fold (dspsr_amd_filterbank* fb, const float* in, uint64_t ics, uint64_t ips, uint64_t in_step,
                                       const int8_t* raw, int layout, float scale, int state, dspsr_amd_fold* fold, uint64_t npart)
{
  Call call ("dspsr_amd_filterbank_perform_fold");
  call.o (fb).p (in).u (ics).u (ips).u (in_step).p (raw);
  if (raw) call.i (layout).f (scale);
  else call.text ("-").text ("-");                                                // (read only with a packed block; the adaptors may leave them unset)
  return call.i (state).o (fold).u (npart).status (fb ? fb->ctx : 0);
}

// ---- detection, scrunching
int dspsr_amd_detect_polarimetry (dspsr_amd_ctx* ctx, int state, uint32_t ndim, const float* in, uint64_t ics, uint64_t ips, float* out,
                                  uint64_t ocs, uint64_t ops, uint32_t nchan, uint64_t ndat)
{
  return Call ("dspsr_amd_detect_polarimetry").c (ctx).i (state).u (ndim).p (in).u (ics).u (ips).p (out).u (ocs).u (ops).u (nchan)
         .u (ndat).status (ctx);
}
int dspsr_amd_detect_square_law (dspsr_amd_ctx* ctx, int intensity, const float* in, uint64_t ics, uint64_t ips, float* out,
                                 uint64_t ocs, uint64_t ops, uint32_t nchan, uint32_t npol, uint64_t ndat)
{
  return Call ("dspsr_amd_detect_square_law").c (ctx).i (intensity).p (in).u (ics).u (ips).p (out).u (ocs).u (ops).u (nchan).u (npol)
         .u (ndat).status (ctx);
}
int dspsr_amd_tscrunch_fpt (dspsr_amd_ctx* ctx, const float* in, uint64_t ics, uint64_t ips, float* out, uint64_t ocs, uint64_t ops,
                            uint32_t nchan, uint32_t npol, uint32_t ndim, uint64_t ndat_in, uint32_t sfactor, float* carry,
                            uint32_t* carry_count, uint64_t* nout)
{
  Call call ("dspsr_amd_tscrunch_fpt");
  call.c (ctx).p (in).u (ics).u (ips).p (out).u (ocs).u (ops).u (nchan).u (npol).u (ndim).u (ndat_in).u (sfactor).p (carry)
      .fmt ("count %u", carry_count ? *carry_count : 0u).fmt ("nout %llu", (unsigned long long) (nout ? *nout : 0));
  return call.status (ctx);
}
int dspsr_amd_fscrunch_fpt (dspsr_amd_ctx* ctx, const float* in, uint64_t ics, uint64_t ips, float* out, uint64_t ocs, uint64_t ops,
                            uint32_t nchan_in, uint32_t npol, uint64_t nfloat, uint32_t sfactor)
{
  return Call ("dspsr_amd_fscrunch_fpt").c (ctx).p (in).u (ics).u (ips).p (out).u (ocs).u (ops).u (nchan_in).u (npol).u (nfloat)
         .u (sfactor).status (ctx);
}

// ---- fold
int dspsr_amd_fold_create (dspsr_amd_ctx* ctx, dspsr_amd_fold** fold)
{
  Call call ("dspsr_amd_fold_create");
  call.c (ctx);
  const int code = call.status (ctx, ctx ? DSPSR_AMD_OK : DSPSR_AMD_EINVAL);
  if (code == DSPSR_AMD_OK)
  { *fold = new dspsr_amd_fold; (*fold)->ord = nfold ++; (*fold)->ctx = ctx; (*fold)->nbin = 0; rec::note ("  = fold%d", (*fold)->ord); }
  return code;
}
void dspsr_amd_fold_destroy (dspsr_amd_fold* fold) { Call ("dspsr_amd_fold_destroy").o (fold).end (); }
int dspsr_amd_fold_bind_profile (dspsr_amd_fold* fold, float* profile, uint64_t span, uint32_t nchan, uint32_t npol, uint32_t ndim,
                                 uint32_t nbin)
{ return Call ("dspsr_amd_fold_bind_profile").o (fold).p (profile).u (span).u (nchan).u (npol).u (ndim).u (nbin).status (fold->ctx); }
int dspsr_amd_fold_set_nbin (dspsr_amd_fold* fold, uint32_t nbin)
{
  Call call ("dspsr_amd_fold_set_nbin");
  call.o (fold).u (nbin);
  const int code = call.status (fold->ctx);
  if (code == DSPSR_AMD_OK) fold->nbin = nbin;
  return code;
}
int dspsr_amd_fold_set_ndat (dspsr_amd_fold* fold, uint64_t ndat, uint64_t idat_start)
{ return Call ("dspsr_amd_fold_set_ndat").o (fold).u (ndat).u (idat_start).status (fold->ctx); }
int dspsr_amd_fold_set_bin (dspsr_amd_fold* fold, uint64_t idat, double ibin, double bins_per_sample)
{ return Call ("dspsr_amd_fold_set_bin").o (fold).u (idat).f (ibin).f (bins_per_sample).status (fold->ctx); }
int dspsr_amd_fold_set_bins (dspsr_amd_fold* fold, double phi, double phase_per_sample, uint64_t ndat, uint64_t idat_start,
                             uint32_t* hits_host, uint64_t* ndat_folded)
{
  Call call ("dspsr_amd_fold_set_bins");
  call.o (fold).f (phi).f (phase_per_sample).u (ndat).u (idat_start).p (hits_host).text (ndat_folded ? "folded" : "null");
  const int code = call.status (fold->ctx);
  if (code == DSPSR_AMD_OK)
  {
    for (uint32_t i = 0; hits_host && i < fold->nbin; i++) hits_host[i] += hits_value;
    if (ndat_folded) *ndat_folded = folded_value;
  }
  return code;
}
uint64_t dspsr_amd_fold_get_ndat_folded (const dspsr_amd_fold* fold)
{
  Call ("dspsr_amd_fold_get_ndat_folded").o (fold).end (std::to_string (folded_value));
  return folded_value;
}
int dspsr_amd_fold_fold (dspsr_amd_fold* fold, const float* in, uint64_t ics, uint64_t ips)
{ return Call ("dspsr_amd_fold_fold").o (fold).p (in).u (ics).u (ips).status (fold->ctx); }
int dspsr_amd_fold_fold_zeroed (dspsr_amd_fold* fold, const float* in, uint64_t ics, uint64_t ips, uint32_t* hits_dev)
{ return Call ("dspsr_amd_fold_fold_zeroed").o (fold).p (in).u (ics).u (ips).p (hits_dev).status (fold->ctx); }

// ---- cyclic fold
int dspsr_amd_cyclic_fold_create (dspsr_amd_ctx* ctx, dspsr_amd_cyclic_fold** fold)
{
  Call call ("dspsr_amd_cyclic_fold_create");
  call.c (ctx);
  const int code = call.status (ctx, ctx ? DSPSR_AMD_OK : DSPSR_AMD_EINVAL);
  if (code == DSPSR_AMD_OK)
  { *fold = new dspsr_amd_cyclic_fold; (*fold)->ord = ncyclic ++; (*fold)->ctx = ctx; rec::note ("  = cyclic%d", (*fold)->ord); }
  return code;
}
void dspsr_amd_cyclic_fold_destroy (dspsr_amd_cyclic_fold* fold) { Call ("dspsr_amd_cyclic_fold_destroy").o (fold).end (); }
int dspsr_amd_cyclic_fold_set_shape (dspsr_amd_cyclic_fold* fold, uint32_t nchan, uint32_t npol_in, uint32_t npol_out, uint32_t nlag,
                                     uint32_t mover, uint32_t nbin)
{ return Call ("dspsr_amd_cyclic_fold_set_shape").o (fold).u (nchan).u (npol_in).u (npol_out).u (nlag).u (mover).u (nbin).status (fold->ctx); }
int dspsr_amd_cyclic_fold_set_ndat (dspsr_amd_cyclic_fold* fold, uint64_t ndat, uint64_t idat_start)
{ return Call ("dspsr_amd_cyclic_fold_set_ndat").o (fold).u (ndat).u (idat_start).status (fold->ctx); }
int dspsr_amd_cyclic_fold_set_bin (dspsr_amd_cyclic_fold* fold, uint64_t idat, double ibin, double bins_per_sample)
{ return Call ("dspsr_amd_cyclic_fold_set_bin").o (fold).u (idat).f (ibin).f (bins_per_sample).status (fold->ctx); }
int dspsr_amd_cyclic_fold_fold (dspsr_amd_cyclic_fold* fold, const float* in, uint64_t ics, uint64_t ips)
{ return Call ("dspsr_amd_cyclic_fold_fold").o (fold).p (in).u (ics).u (ips).status (fold->ctx); }
int dspsr_amd_cyclic_fold_zero (dspsr_amd_cyclic_fold* fold) { return Call ("dspsr_amd_cyclic_fold_zero").o (fold).status (fold->ctx); }
int dspsr_amd_cyclic_fold_synch_lags (dspsr_amd_cyclic_fold* fold, float* lagdata_host)
{ return Call ("dspsr_amd_cyclic_fold_synch_lags").o (fold).p (lagdata_host).status (fold->ctx); }

// ---- spectral kurtosis
int dspsr_amd_sk_limits (uint32_t M, uint32_t std_devs, float* lower, float* upper)
{
  Call call ("dspsr_amd_sk_limits");
  call.u (M).u (std_devs);
  *lower = 0.5f; *upper = 1.5f;
  return call.status (0);
}
int dspsr_amd_sk_create (dspsr_amd_ctx* ctx, dspsr_amd_sk** out)
{
  Call call ("dspsr_amd_sk_create");
  call.c (ctx);
  const int code = call.status (ctx, ctx ? DSPSR_AMD_OK : DSPSR_AMD_EINVAL);
  if (code == DSPSR_AMD_OK)
  {
    dspsr_amd_sk* sk = new dspsr_amd_sk;
    sk->ord = nsk ++; sk->ctx = ctx;
    sk->estimates = allocate (4096); sk->zapmask = allocate (4096);            // (the scenarios' shapes are far smaller)
    rec::note ("  = sk%d, estimates b%d, zapmask b%d", sk->ord, buffers[buffers.size () - 2].ord, buffers.back ().ord);
    *out = sk;
  }
  return code;
}
void dspsr_amd_sk_destroy (dspsr_amd_sk* sk) { Call ("dspsr_amd_sk_destroy").o (sk).end (); }
int dspsr_amd_sk_set_shape (dspsr_amd_sk* sk, uint32_t nchan, uint32_t npol, uint32_t M)
{ return Call ("dspsr_amd_sk_set_shape").o (sk).u (nchan).u (npol).u (M).status (sk->ctx); }
int dspsr_amd_sk_set_options (dspsr_amd_sk* sk, uint32_t std_devs, uint32_t chan_start, uint32_t chan_end, int no_fscr, int no_tscr,
                              int no_ft)
{ return Call ("dspsr_amd_sk_set_options").o (sk).u (std_devs).u (chan_start).u (chan_end).i (no_fscr).i (no_tscr).i (no_ft).status (sk->ctx); }
int dspsr_amd_sk_compute (dspsr_amd_sk* sk, const float* in, uint64_t cs, uint64_t ps, uint64_t ndat)
{ return Call ("dspsr_amd_sk_compute").o (sk).p (in).u (cs).u (ps).u (ndat).status (sk->ctx); }
int dspsr_amd_sk_reset_mask (dspsr_amd_sk* sk) { return Call ("dspsr_amd_sk_reset_mask").o (sk).status (sk->ctx); }
int dspsr_amd_sk_detect_tscr (dspsr_amd_sk* sk, float lower, float upper)
{ return Call ("dspsr_amd_sk_detect_tscr").o (sk).f (lower).f (upper).status (sk->ctx); }
int dspsr_amd_sk_detect_skfb (dspsr_amd_sk* sk, float lower, float upper)
{ return Call ("dspsr_amd_sk_detect_skfb").o (sk).f (lower).f (upper).status (sk->ctx); }
int dspsr_amd_sk_detect_fscr (dspsr_amd_sk* sk) { return Call ("dspsr_amd_sk_detect_fscr").o (sk).status (sk->ctx); }
int dspsr_amd_sk_mask (dspsr_amd_sk* sk, const float* in, uint64_t ics, uint64_t ips, float* out, uint64_t ocs, uint64_t ops)
{ return Call ("dspsr_amd_sk_mask").o (sk).p (in).u (ics).u (ips).p (out).u (ocs).u (ops).status (sk->ctx); }
uint64_t dspsr_amd_sk_npart (dspsr_amd_sk* sk)
{
  Call ("dspsr_amd_sk_npart").o (sk).end (std::to_string (sk_npart_value));
  return sk_npart_value;
}
float* dspsr_amd_sk_estimates_dev (dspsr_amd_sk* sk)
{
  Call ("dspsr_amd_sk_estimates_dev").o (sk).end (pointer_text (sk->estimates));
  return (float*) sk->estimates;
}
uint8_t* dspsr_amd_sk_zapmask_dev (dspsr_amd_sk* sk)
{
  Call ("dspsr_amd_sk_zapmask_dev").o (sk).end (pointer_text (sk->zapmask));
  return (uint8_t*) sk->zapmask;
}

}
