// dspsr_amd_adaptor_common.h -- what the adaptor headers of this directory share: the status-to-Error mapping, the row geometry
// of a TimeSeries as the C-ABI takes it, and device scratch owned by an engine.  It includes no dsp header (the templates
// take the series type from their caller), so every adaptor header can include it.
#ifndef DSPSR_AMD_ADAPTOR_COMMON_H
#define DSPSR_AMD_ADAPTOR_COMMON_H

#include "Error.h"

#include "dspsr_amd.h"

namespace HIP
{
  //! every non-zero C-ABI status is rethrown as the reference's `Error` with the library's message: EINVAL as InvalidParam,
  //! anything else as InvalidState.  The message is data, never a format.  `without_ctx`: the text of an engine that words the
  //! missing context itself (the library says "null context")
  inline void check (dspsr_amd_ctx* ctx, int status, const char* method, const char* without_ctx = 0)
  {
    if (status != DSPSR_AMD_OK)
      throw Error (status == DSPSR_AMD_EINVAL ? InvalidParam : InvalidState, method, "%s",
                   !ctx && without_ctx ? without_ctx : dspsr_amd_last_error (ctx));
  }

  //! FPT rows as the C-ABI takes them: get_datptr (ichan, ipol) = base + ichan * cs + ipol * ps (floats)
  template <class Ptr> struct Rows { Ptr base; uint64_t cs, ps; };

  //! the rows of a dsp::TimeSeries (Series = [const] dsp::TimeSeries; a template only so that this header needs no dsp
  //! header).  A stride exists only between rows that exist: `nchan` and `npol` say how many the caller walks, and are the
  //! series' own unless the call site says otherwise
  template <class Series>
  Rows<decltype (((Series*) 0)->get_datptr (0, 0))> rows_of (Series* series, unsigned nchan, unsigned npol)
  {
    Rows<decltype (series->get_datptr (0, 0))> rows;
    rows.base = series->get_datptr (0, 0);
    rows.cs = nchan > 1 ? series->get_datptr (1, 0) - rows.base : 0;
    rows.ps = npol > 1 ? series->get_datptr (0, 1) - rows.base : 0;
    return rows;
  }
  template <class Series>
  Rows<decltype (((Series*) 0)->get_datptr (0, 0))> rows_of (Series* series)
  { return rows_of (series, series->get_nchan (), series->get_npol ()); }

  //! device scratch of one engine: replaced when its owner asks for another size, freed with it
  class DeviceScratch
  {
  public:
    DeviceScratch (dspsr_amd_ctx* _ctx) : ctx (_ctx), ptr (0), count (0) { }
    ~DeviceScratch () { release (); }
    void* get () const { return ptr; }
    //! elements, as the owner counts them
    uint64_t size () const { return count; }
    //! a new buffer of `_count` elements of `element` bytes in the place of the old one
    void replace (uint64_t _count, size_t element, bool zeroed, const char* method)
    {
      if (ptr) check (ctx, dspsr_amd_free (ctx, ptr), method);
      ptr = 0; count = 0;
      void* p = 0;
      check (ctx, dspsr_amd_malloc (ctx, _count * element, &p), method);
      if (zeroed) check (ctx, dspsr_amd_zero (ctx, p, _count * element), method);
      ptr = p; count = _count;
    }
    //! for a destructor that must free before it destroys a library object
    void release () { if (ptr) dspsr_amd_free (ctx, ptr); ptr = 0; count = 0; }
  private:
    DeviceScratch (const DeviceScratch&);
    DeviceScratch& operator= (const DeviceScratch&);
    dspsr_amd_ctx* ctx;
    void* ptr;
    uint64_t count;
  };
}

#endif
