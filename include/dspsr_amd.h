/* dspsr_amd.h -- C-ABI of the MI355X (gfx950) coherent-dedispersion + detection + fold engine.
 *
 * This is the drop-in boundary for DSPSR's GPU hot path.  Each entry point replaces one method of
 * the reference's Engine plug-in interfaces (citations are relative to the demorest/dspsr tree):
 *
 *   dsp::Memory                 Kernel/Classes/dsp/Memory.h:18-34      (CUDA impl MemoryCUDA.C:47-106)
 *   dsp::Filterbank::Engine     Signal/General/dsp/FilterbankEngine.h:15-44 (CUDA impl FilterbankCUDA.cu:73-304)
 *   dsp::Detection::Engine      Signal/General/dsp/Detection.h:98-106  (CUDA impl DetectionCUDA.cu:127-322)
 *   dsp::Fold::Engine           Signal/Pulsar/dsp/Fold.h:249-312       (CUDA impl FoldCUDA.cu:64-697)
 *   dsp::CyclicFoldEngine       Signal/Pulsar/dsp/CyclicFold.h:93-160  (CPU impl CyclicFold.C:173-555: the definition;
 *                                                                       CUDA impl CyclicFoldEngineCUDA.cu)
 *   host-side preparation       Dedispersion.C:216-556, Response.C:132-344,649-700, optimize_fft.c:63-127,
 *                               Filterbank.C:55-263, Fold.C:650-787
 *
 * Conventions: plain C, opaque handles, every function returns 0 on success or a negative
 * DSPSR_AMD_E* code (never throws); dspsr_amd_last_error() gives the text a host wrapper turns
 * into the reference's `Error` exception.  All device work is enqueued on the context's HIP
 * stream and is asynchronous unless stated; pointers named *_dev are device pointers.
 * The host adaptor classes that bind these to the dsp::*::Engine interfaces are in
 * dspsr_amd/host/ (see INTEGRATION.md).
 */
#ifndef DSPSR_AMD_H
#define DSPSR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSPSR_AMD_OK 0
#define DSPSR_AMD_EINVAL (-1)   /* invalid argument / unsupported configuration (reference: Error InvalidParam/InvalidState) */
#define DSPSR_AMD_EHIP (-2)     /* HIP runtime failure (reference: CUFFTError / check_error) */
#define DSPSR_AMD_ENOMEM (-3)
#define DSPSR_AMD_ESTATE (-4)   /* called out of order (e.g. perform before set_kernel) */

typedef struct dspsr_amd_ctx dspsr_amd_ctx;
typedef struct dspsr_amd_filterbank dspsr_amd_filterbank;
typedef struct dspsr_amd_fold dspsr_amd_fold;
typedef struct dspsr_amd_cyclic_fold dspsr_amd_cyclic_fold;
typedef struct dspsr_amd_plfb dspsr_amd_plfb;

/* ---- context: one per pipeline thread / GPU, bound to one stream (SingleThread.C:213-290) ---- */
/* hip_stream: a hipStream_t to enqueue on (NULL = the legacy default stream), or
 * DSPSR_AMD_NEW_STREAM to let the context create and own a non-blocking stream */
#define DSPSR_AMD_NEW_STREAM ((void*)(intptr_t)-1)
int dspsr_amd_ctx_create(int device, void* hip_stream, dspsr_amd_ctx** ctx);
void dspsr_amd_ctx_destroy(dspsr_amd_ctx* ctx);
const char* dspsr_amd_last_error(const dspsr_amd_ctx* ctx);
int dspsr_amd_stream_sync(dspsr_amd_ctx* ctx);            /* FilterbankEngine::finish / check_error_stream */
const char* dspsr_amd_version(void);
/* sha256 (12 hex digits) of the sources the loaded library was built from (dspsr_amd/csrc/Makefile: BUILD_ID); the evidence files
 * under profiles/ and the bench line name it, so that a counter profile can be matched to the library that was timed */
const char* dspsr_amd_build_id(void);

/* ---- dsp::Memory (Memory.h:18-34): do_allocate / do_free / do_zero / do_copy ---- */
int dspsr_amd_malloc(dspsr_amd_ctx* ctx, size_t nbytes, void** ptr_dev);
int dspsr_amd_free(dspsr_amd_ctx* ctx, void* ptr_dev);
int dspsr_amd_zero(dspsr_amd_ctx* ctx, void* ptr_dev, size_t nbytes);
#define DSPSR_AMD_H2D 1
#define DSPSR_AMD_D2H 2
#define DSPSR_AMD_D2D 3
int dspsr_amd_copy(dspsr_amd_ctx* ctx, void* dst, const void* src, size_t nbytes, int kind);

/* ---- dsp::TimeSeries::Engine::copy_data_fpt (Kernel/Classes/dsp/TimeSeries.h:211-223; CUDA twin
 * Kernel/Classes/TimeSeriesCUDA.cu:20-29,75-200): device-to-device copy of `nfloat` floats of every
 * (channel, polarisation) row -- the overlap carry-over of dsp::InputBuffering (InputBuffering.C:35-126) and
 * TimeSeries::prepend.  Strides in floats between channel rows / polarisation rows; the row pointers already
 * include the start sample.  Rows of `to` and `from` must not overlap: DSPSR_AMD_EINVAL (with a message, nothing launched) when
 * a row of `to` shares a float with a row of `from` -- decided exactly when both sides have the same strides (a move inside one
 * buffer), and by the spans [first row start, last row end) of the two sides otherwise. */
int dspsr_amd_copy_fpt(dspsr_amd_ctx* ctx, float* to_dev, uint64_t to_chan_stride, uint64_t to_pol_stride,
                       const float* from_dev, uint64_t from_chan_stride, uint64_t from_pol_stride,
                       uint32_t nchan, uint32_t npol, uint64_t nfloat);
/* dsp::TimeSeries::operator += on device rows (Kernel/Classes/TimeSeries.C, used by PhaseSeries::combine,
 * Signal/Pulsar/PhaseSeries.C:442-484): to[row][i] += from[row][i]; same row geometry arguments as copy_fpt.  The profile
 * half of combining two device-resident PhaseSeries (the hits / integration_length half stays with the host object). */
int dspsr_amd_add_fpt(dspsr_amd_ctx* ctx, float* to_dev, uint64_t to_chan_stride, uint64_t to_pol_stride,
                      const float* from_dev, uint64_t from_chan_stride, uint64_t from_pol_stride,
                      uint32_t nchan, uint32_t npol, uint64_t nfloat);

/* ---- dsp::Filterbank::Engine ------------------------------------------------------------
 * setup(Filterbank*)  -> dspsr_amd_filterbank_create + dspsr_amd_filterbank_set_kernel
 *   (FilterbankCUDA.cu:73-168 reads freq_res, nchan_subband, input state, response nchan/ndat/
 *    impulse_pos/neg and copies the host-built, already swapped kernel to the device) */
typedef struct {
  uint32_t nchan_subband;   /* output channels per input channel          Filterbank.C:68
                               2^k, or 2^k times an odd R <= 127 (dspsr -F 96:D, -F 400:D, -F 1000:D, -F 25:D: the reference plans any
                               length, Filterbank.C:107-155; here the forward transform of R interleaved power-of-two
                               sub-sequences + one radix-R step -- kernels of their own for R = 3, 5, 7, 9, 15, a run-time-radix
                               form for the others; freq_res <= 8192 then) */
  uint32_t freq_res;        /* response ndat = backward FFT length                            Filterbank.C:93
                               1: the NON-CONVOLVING filterbank of `dspsr -F N` (Filterbank::Config::After / Never; Filterbank.C:614-623,
                               FilterbankCUDA.cu:92-116 with plan_bwd == NULL): one nchan_subband-point forward transform per output
                               sample, no backward transform, nkeep = 1, no overlap (nfilt_pos = nfilt_neg = 0); nchan_subband 2^k in
                               [2, 8192]; a kernel of input_nchan * nchan_subband factors is applied if set (Response::operate); one
                               launch, no scratch (csrc/fb_plain.hip).  dsp::Convolution then runs on its output as a second object
                               with nchan_subband = 1.
                               2^k >= 2, or 2^k times an odd R <= 127 (dspsr -x 12288, -x 11264): bins R m' + r of a channel are R
                               pseudo-channels of freq_res / R bins through the power-of-two passes, one radix-R step in time adds
                               their transforms (a pass of its own: fold_is_fused() == 0; freq_res / R <= 8192).  Both lengths may
                               carry an odd factor when the product of the two stays <= 127 (-F 96:D -x 768) */
  uint32_t nfilt_pos;       /* response impulse_pos                       Filterbank.C:90  */
  uint32_t nfilt_neg;       /* response impulse_neg                       Filterbank.C:91  */
  uint32_t input_nchan;     /* input channels (kernel has input_nchan*nchan_subband*freq_res bins) */
  uint32_t npol;            /* 1 or 2 */
  uint32_t real_input;      /* 1: Signal::Nyquist (ndim 1), 0: Signal::Analytic (ndim 2) */
  uint32_t max_parts;       /* parts processed per launch group (scratch is sized for this); 0 => default */
  uint32_t force_four_pass; /* 0 => passes chosen from the geometry; 1: two-pass inverse (the path of freq_res > 8192 and of
                               dsp::Convolution) also where the single-pass inverse would do -- and instead of the one-pass /
                               three-pass convolution; 2: never the two-pass path of short responses (complex dual-pol input,
                               nchan_subband * freq_res^2 <= 2^27: forward and inverse transforms in two tiles), the one-pass /
                               three-pass convolution or the grouping of a convolution's channels; same results to rounding in every case */
  uint32_t fused_fold;      /* dspsr_amd_filterbank_perform_fold: DSPSR_AMD_FUSED_AUTO (fold inside the last filterbank
                               pass when the channel tiles fill the chip), _ALWAYS, _NEVER -- same sums bit for bit */
  uint32_t split_in_inverse; /* 0 => real dual-polarisation input on the three-pass path: the forward row pass forms the Hermitian
                               split and stores the two polarisations, the inverse pass loads them ready
                               (dspsr_amd_filterbank_presplit() == 1); 1: the inverse pass splits, as it does for every other
                               input and path (comparison runs and tests) -- the same numbers bit for bit */
} dspsr_amd_filterbank_config;
#define DSPSR_AMD_FUSED_AUTO 0
#define DSPSR_AMD_FUSED_ALWAYS 1
#define DSPSR_AMD_FUSED_NEVER 2

int dspsr_amd_filterbank_create(dspsr_amd_ctx* ctx, const dspsr_amd_filterbank_config* cfg,
                                dspsr_amd_filterbank** fb);
void dspsr_amd_filterbank_destroy(dspsr_amd_filterbank* fb);
/* host kernel: input_nchan*nchan_subband*freq_res complex floats (response->get_datptr(0,0)); NULL => no response */
int dspsr_amd_filterbank_set_kernel(dspsr_amd_filterbank* fb, const float* kernel_host, uint64_t ncomplex);
/* Matrix response (`dspsr -pac`: PolnCalibration x Dedispersion as a ResponseProduct, LoadToFold1.C:270-289; Filterbank.C:186-206
 * matrix_convolution = response->get_ndim() == 8): one Jones matrix per bin, applied to the spectra d1, d2 of the two polarisations
 * inside the inverse pass, where the scalar response multiplies them (Response::operate(data1, data2), Response.C:515-585):
 *     d1' = f11*d1 + f12*d2      d2' = f21*d1 + f22*d2
 * response_host: nmatrix = nchan_subband*freq_res matrices of 8 floats in the reference's element order f11, f21, f22, f12
 * (Response::set(vector<Jones>), Response.C:614-640), bin k of output channel k / freq_res -- response->get_datptr(0,0) of an
 * ndim 8 Response.  The product with the dedispersion chirp is the caller's (Response::operator*=, Response.C:73-104).
 * Each output is the scalar path's complex multiply of its own polarisation with the diagonal element, then the other
 * polarisation's two real products added one after the other (Response.C:570-582), so diag(k, k) gives the bits of set_kernel(k).
 * set_response_matrix and set_kernel replace each other; set_kernel(fb, NULL, 0) clears either.
 * Accepted objects (else DSPSR_AMD_EINVAL with the limit's name, before any allocation; the object keeps what it had):
 *   npol == 2; input_nchan == 1 (the reference throws for more, Filterbank.C:199-201); nchan_subband >= 2 and
 *   2 <= freq_res <= 8192, both powers of two; force_four_pass != 1; real or complex input, split_in_inverse 0 or 1.
 * With a matrix response every perform entry point works; a geometry of the two-pass path takes the three passes
 * (dspsr_amd_filterbank_npass() == 3), and perform_fold / perform_search run through the object's internal detected block
 * (fold_is_fused() == 0, search_is_fused() == 0).  The response is streamed per part by the inverse pass: 32 bytes per bin. */
int dspsr_amd_filterbank_set_response_matrix(dspsr_amd_filterbank* fb, const float* response_host, uint64_t nmatrix);
/* Response::get_ndim of what the object holds: 0 none (or not set), 2 complex (set_kernel), 8 Jones (set_response_matrix) */
int dspsr_amd_filterbank_response_ndim(const dspsr_amd_filterbank* fb);
/* derived sizes, same arithmetic as Filterbank::make_preparations (Filterbank.C:107-155) */
int dspsr_amd_filterbank_sizes(const dspsr_amd_filterbank* fb, uint64_t* nsamp_fft, uint64_t* nsamp_overlap,
                               uint64_t* nsamp_step, uint32_t* nkeep);

/* perform(in, out, npart, in_step, out_step)  (FilterbankEngine.h:28-32, FilterbankCUDA.cu:181-304)
 *   in_dev : unpacked float32 rows, in->get_datptr(ichan,ipol) = in_dev + ichan*in_chan_stride + ipol*in_pol_stride (floats)
 *   out_dev: complex float rows, out->get_datptr(ochan,ipol) = out_dev + ochan*out_chan_stride + ipol*out_pol_stride (floats);
 *            NULL => benchmark only (FilterbankCUDA.cu:265)
 *   in_step: floats between parts (= nsamp_step*ndim), out_step: floats between parts (= 2*nkeep)
 * The output (perform and perform_raw alike): part k of row (ochan, ipol) is the 2*nkeep floats at row + k*out_step.  out_dev may be
 * any float-aligned address -- dsp::TimeSeries rows start at buffer + reserve, as a rule 8-byte and seldom 16-byte aligned -- and the
 * strides any number of floats; no writer asks for more.  out_step >= 2*nkeep (larger: the floats between two parts are not
 * written), and the rows must not overlap: with row = (npart-1)*out_step + 2*nkeep either out_pol_stride >= row and
 * out_chan_stride >= (npol-1)*out_pol_stride + row (FPT order), or out_chan_stride >= row and out_pol_stride >=
 * (nchan-1)*out_chan_stride + row.  Anything else is refused with DSPSR_AMD_EINVAL before a launch.  Only the floats of the parts are
 * written: nothing in front of a row, between parts, behind a row (tests/test_gpu_output_forms.py). */
int dspsr_amd_filterbank_perform(dspsr_amd_filterbank* fb, const float* in_dev, uint64_t in_chan_stride,
                                 uint64_t in_pol_stride, float* out_dev, uint64_t out_chan_stride,
                                 uint64_t out_pol_stride, uint64_t npart, uint64_t in_step, uint64_t out_step);

/* Optional side channel (north star: fuse the 8-bit load into FFT pass 1; replaces the separate
 * unpack kernels GenericEightBitUnpackerCUDA.cu:24-45 / CASPSRUnpackerCUDA.cu:44-82 + perform).
 * raw_dev points at the first byte of the block (BitSeries::get_rawptr()); value = (int8+0.5)*scale. */
#define DSPSR_AMD_RAW_GENERIC 0  /* byte ((t*nchan+c)*npol+p)*ndim+d   BitUnpacker.C:48-80 */
#define DSPSR_AMD_RAW_CASPSR 1   /* 4 B pol0, 4 B pol1 repeating       CASPSRUnpacker.C:132-187; the block starts on a group
                                    boundary and holds whole 8-byte groups: ceil(nsamp/4)*8 bytes */
#define DSPSR_AMD_RAW_UWB16 2    /* 16-bit offset-binary complex, 2048-sample blocks per polarisation, single channel;
                                    value = float(int16(x ^ 0x8000)) * scale   uwb/UWBUnpackerCUDA.cu:24-75,
                                    uwb/UWBUnpacker.C:196-207 (the reference applies no scale: pass 1.0) */
/* MeerKAT beamformer heaps (INSTRUMENT MKBF / MKBFRo, kat/MeerKATUnpacker.C:137-230): complex 8-bit, npol 1 | 2, any nchan.  A
 * block is whole heaps of 256 samples; heap h holds, for pol in order and then chan in order, the 256 consecutive (int8 re, int8 im)
 * pairs of that (chan, pol) -- 512 contiguous bytes per run:
 *     byte of stored sample s of heap h = (((h * npol + pol) * nchan + chan) * 256 + s) * 2 + d
 * Stream sample t of a row is stored at s = t & 255 of heap t >> 8; DSPSR_AMD_RAW_MEERKAT_SWAP (MKBFRo, sample_swap = 2) exchanges
 * odd and even samples: s = (t & 255) ^ 1.  Overlap-save parts are nsamp_step samples apart and blocks overlap, so a block does
 * not start on a heap boundary in general: raw_dev points at the first byte of the HEAP that holds the call's first sample, and the
 * layout word carries first_sample, the index inside that heap of stream sample 0 of the call (stateless; heap layouts only: a
 * first_sample on any other layout, or one above 255, is DSPSR_AMD_EINVAL).  The block holds ceil((first_sample + nsamp) / 256)
 * whole heaps.  raw_dev must be 16-byte aligned (every run of a heap then is): anything else is DSPSR_AMD_EINVAL before a launch. */
#define DSPSR_AMD_RAW_MEERKAT 3
#define DSPSR_AMD_RAW_MEERKAT_SWAP 4
#define DSPSR_AMD_RAW_AT(layout, first_sample) ((layout) | ((first_sample) << 8))
/* out_dev, its strides and out_step: as dspsr_amd_filterbank_perform, the same checks */
int dspsr_amd_filterbank_perform_raw(dspsr_amd_filterbank* fb, const int8_t* raw_dev, int raw_layout, float scale,
                                     float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride,
                                     uint64_t npart, uint64_t out_step);

/* Fused filterbank + Detection::polarimetry (npol must be 2): writes the detected TimeSeries directly.
 *   state: DSPSR_AMD_COHERENCE | DSPSR_AMD_STOKES ; ndim in {1,2,4} (Detection.C:423-474 layouts):
 *     ndim 4: det_dev + chan*det_chan_stride + 4*idat               (npol 1)
 *     ndim 2: det_dev + chan*det_chan_stride + plane*det_pol_stride + 2*idat   (plane0 = PP,QQ plane1 = Re,Im)
 *     ndim 1: det_dev + chan*det_chan_stride + k*det_pol_stride + idat         (k = 0..3)
 *   exactly one of in_f32_dev / raw_dev is non-NULL.
 * det_dev may be any float-aligned address and the strides any number of floats (the float4 / float2 samples of ndim 4 / 2 are
 * written at whatever address that gives).  A detected row is npart*nkeep*ndim floats; the 4/ndim rows of a channel and the
 * channels must not overlap, in one of two orders: channel-major (TimeSeries FPT order: det_pol_stride >= row, det_chan_stride >=
 * (4/ndim - 1)*det_pol_stride + row) or plane-major (det_chan_stride >= row, det_pol_stride >= (nchan-1)*det_chan_stride + row).
 * Anything else is refused with DSPSR_AMD_EINVAL before a launch; nothing outside the rows is written.
 *   state: DSPSR_AMD_INTENSITY | DSPSR_AMD_PPQQ (dspsr -d 1, -d 2: Detection::square_law, Detection.C:218-320) ; ndim must be 1:
 *     det_dev + chan*det_chan_stride + q*det_pol_stride + idat    (q < npol_out: 1 for Intensity, 2 for PPQQ)
 *   in the same two row orders.  An object of ONE polarisation takes Intensity alone and yields PP, the power of its polarisation.
 *   Three-pass and two-pass geometries detect inside the inverse pass (the search epilogue of perform_search with a scrunch factor
 *   of 1); the others write their complex rows to a block owned by the object and run dspsr_amd_detect_square_law on it.  Either
 *   way the rows are bit for bit dspsr_amd_filterbank_perform(_raw) followed by dspsr_amd_detect_square_law. */
#define DSPSR_AMD_COHERENCE 0
#define DSPSR_AMD_STOKES 1
int dspsr_amd_filterbank_perform_detect(dspsr_amd_filterbank* fb, const float* in_f32_dev, uint64_t in_chan_stride,
                                        uint64_t in_pol_stride, uint64_t in_step, const int8_t* raw_dev,
                                        int raw_layout, float scale, int state, uint32_t ndim, float* det_dev,
                                        uint64_t det_chan_stride, uint64_t det_pol_stride, uint64_t npart);

/* Fused Filterbank -> Detection -> Fold: the detected time series never leaves the chip.  The profile of `fold` is
 * either npol 1 x ndim 4 (one (PP, QQ, Re, Im) float4 per bin: Detection's CPU default, LoadToFoldConfig.C:104) or
 * npol 2 x ndim 2 (rows (PP, QQ) and (Re, Im) per channel: what the reference's GPU pipeline detects and folds,
 * LoadToFold1.C:1105-1109, DetectionCUDA.cu:145-149) -- the same sums in either shape.  Replaces the chain Filterbank::Engine::perform (FilterbankCUDA.cu:181-304) + Detection::Engine::polarimetry
 * (DetectionCUDA.cu:127-177) + Fold::Engine::fold (FoldCUDA.cu:586-697) for one block of `npart` parts.
 * The bin plan of the npart*nkeep output samples of this call must have been handed to `fold` beforehand
 * (dspsr_amd_fold_set_nbin / set_ndat / set_bin(s) with sample indices counted from the first output sample of
 * this call); it is consumed.  Sums are accumulated into the device profile of `fold` in time order per
 * (chan, bin), bit-identical to perform_detect followed by dspsr_amd_fold_fold.
 * dspsr_amd_filterbank_fold_is_fused() says how this object folds (fused_fold = DSPSR_AMD_FUSED_AUTO):
 *   1  inside the last filterbank pass, one workgroup per tile of channels walking the parts in order (three-pass geometry
 *      with at least one tile per compute unit): exact time-order sums, bit-identical to Detection + Fold;
 *   2  inside the last pass with the parts of a launch cut into runs folded by different workgroups (8 .. ncu-1 tiles):
 *      run 0 continues the profile, the other runs go to partial profiles added in run order after the launch -- sums
 *      re-associated per run, equal to the time-order sums to float rounding, deterministic;
 *   3  four-pass geometry (freq_res > 8192, dsp::Convolution shapes) and phase bins of >= 64 samples: the second inverse pass
 *      reduces every run of 32 consecutive output samples it holds to (at most two) piece sums, a second kernel adds the
 *      pieces of each (channel, bin) in time order -- re-associated like the long-run fold (fold.hip), deterministic; the
 *      detected time series never reaches HBM.  Plans that do not qualify (narrow bins, zero weights, partial folds) take 0;
 *   0  Detection and Fold as separate launches on a block owned by the filterbank object (fewer than 8 tiles,
 *      DSPSR_AMD_FUSED_NEVER, or what the other modes turn down; and every dsp::Convolution object whose float32 rows run in one
 *      or three tile passes -- complex input, two polarisations, 64 <= freq_res <= 2^21: Detection in their last pass).  Three-pass plans with runs of >= 640 samples per bin
 *      take this path too (fold.hip).
 * DSPSR_AMD_FUSED_ALWAYS forces mode 1 on any three-pass geometry.
 *
 * state DSPSR_AMD_INTENSITY | DSPSR_AMD_PPQQ (dspsr -d 1, -d 2): the profile of `fold` is npol 1 x ndim 1 (Intensity; PP of an
 * object of one polarisation) or npol 2 x ndim 1 (PPQQ: the rows PP and QQ of a channel); any other pairing of state and shape is
 * DSPSR_AMD_EINVAL with a message that names both.  The sums are those of perform_detect(state) followed by dspsr_amd_fold_fold:
 * bit for bit in modes 1 and 0, the run-wise re-association above in mode 2.  dspsr_amd_filterbank_fold_is_fused_state(fb, state)
 * says how the object folds `state`: for Coherence and Stokes what dspsr_amd_filterbank_fold_is_fused says; for the two square-law
 * states 1, 2 (k_inv_chan<., 3 | 7, .>: a sample is staged as one or two floats and added to scalar accumulators, so a bound
 * profile fuses at ANY float-aligned address, span and padding) or 0 -- never 3: four-pass objects and calls that take the
 * two-pass path (generic 8-bit complex blocks, npass(1) == 2) run Detection and Fold as launches of their own.  An object of
 * one polarisation fuses like one of two. */
int dspsr_amd_filterbank_fold_is_fused(const dspsr_amd_filterbank* fb);
int dspsr_amd_filterbank_fold_is_fused_state(const dspsr_amd_filterbank* fb, int state);
/* How many transform passes (trips of the part through HBM scratch + 1) a call makes -- the role of the plan choice inside
 * CUDA::FilterbankEngine::setup (FilterbankCUDA.cu:92-116: one forward and one batched backward cuFFT plan).  raw_input != 0:
 * the answer for dspsr_amd_filterbank_perform_raw / _detect / _fold on a generic 8-bit block, else for float32 rows.
 *   1  freq_res = 1: the non-convolving filterbank, one tile pass from the input to the output rows; and (raw_input == 0)
 *      dsp::Convolution shapes -- nchan_subband = 1, complex input with two polarisations -- with 64 <= freq_res <= 8192 on float32
 *      rows: forward transform, response, backward transform, keep window and Detection of a (channel, part) sequence in ONE tile
 *      (csrc/fb_conv1.hip; force_four_pass != 0 keeps the four passes);
 *   2  short responses: complex dual-pol 8-bit input with 512 <= freq_res <= 4096 and 2^13 / freq_res <= nchan_subband <=
 *      2^27 / freq_res^2 (upper end: one 50 MHz sub-band with -F 512:D -x 512): column forward pass, then rows + chirp + inverse
 *      transforms in ONE tile -- the spectrum stays on chip;
 *   3  forward columns, forward rows, inverse per channel (freq_res <= 8192); and (raw_input == 0) the dsp::Convolution shapes above
 *      with 2^14 <= freq_res <= 2^21 on float32 rows: the forward transform's second pass and the inverse transform's first one run
 *      along the same rows of the spectrum and are ONE pass, the spectrum never reaches memory (csrc/fb_conv3.hip;
 *      force_four_pass != 0 keeps the four passes);
 *   4  two-pass inverse (freq_res > 8192, dsp::Convolution shapes, force_four_pass = 1).  dsp::Convolution on >= 4 complex channels
 *      of float32 rows runs GROUPS of channels as one launch group (forward passes per channel, inverse passes of a group-wide
 *      filterbank: the same numbers bit for bit; force_four_pass = 2 keeps the loop over the channels).
 * The count is that of the TILE passes.  Lengths with an odd factor run the three tile passes per power-of-two sub-sequence and
 * add trips through HBM outside the tiles: nchan_subband = R * 2^k a de-interleave of the input (k_sub_split) and one radix-R pass
 * over the spectrum (k_sub_combine); freq_res = R * 2^k a radix-R pass over the pseudo-channels' time series as well
 * (k_time_combine, with Detection and Fold as launches of their own: fold_is_fused() == 0). */
int dspsr_amd_filterbank_npass(const dspsr_amd_filterbank* fb, int raw_input);
/* 1: perform_raw / _detect / _fold / _search of this object read a block of heaps (DSPSR_AMD_RAW_MEERKAT / _SWAP) inside their one
 * tile pass (csrc/fb_conv1.hip, the 8-bit load decoded in the tile's first stage) -- the dsp::Convolution shapes that run in one
 * pass on float32 rows: nchan_subband = 1, complex input, two polarisations, 64 <= freq_res <= 8192, force_four_pass = 0.  Bit for
 * bit dspsr_amd_unpack_heaps_fpt followed by the float32 entry points.  0: every other object; it refuses heap layouts with
 * DSPSR_AMD_EINVAL naming the limit -- unpack first and hand the float rows over. */
int dspsr_amd_filterbank_takes_heaps(const dspsr_amd_filterbank* fb);
/* 1: the object's three passes run on the pre-split spectrum (dspsr_amd_filterbank_config::split_in_inverse), else 0 */
int dspsr_amd_filterbank_presplit(const dspsr_amd_filterbank* fb);
int dspsr_amd_filterbank_perform_fold(dspsr_amd_filterbank* fb, const float* in_f32_dev, uint64_t in_chan_stride,
                                      uint64_t in_pol_stride, uint64_t in_step, const int8_t* raw_dev, int raw_layout,
                                      float scale, int state, dspsr_amd_fold* fold, uint64_t npart);

/* ---- digifil with a convolving filterbank, `digifil -F N:D [-x M] -t T` (Signal/General/LoadToFil.C:185-222,250-304) ---------
 * One launch group for dsp::Filterbank (+ Dedispersion response) -> dsp::Detection::square_law (Detection.C:218-320: Intensity
 * = (Re0^2 + Im0^2) + (Re1^2 + Im1^2), or PPQQ) -> dsp::TScrunch, FPT branch (TScrunch.C:128-178): the detected rows are never
 * written at the filterbank's output rate.  The npart * nkeep detected samples of every channel continue a STREAM: TScrunch's
 * input buffering re-presents the ndat % tscrunch left-over samples in front of the next block (TScrunch.C:110-111); here the
 * partial sum of those samples stays in carry_dev -- the same sequential sum, out = in[0]; out += in[1]; ... , bit for bit.
 *   out_state       DSPSR_AMD_INTENSITY (npol_out 1) | DSPSR_AMD_PPQQ (npol_out 2) | DSPSR_AMD_COHERENCE (npol_out 4: rows PP, QQ,
 *                   Re PQ*, Im PQ* -- digifits -p 4, digifil -d 4; cross_detect.ic:23-43 as perform_detect(COHERENCE, ndim 1) rounds
 *                   them).  PPQQ and Coherence need two polarisations; DSPSR_AMD_STOKES is refused by name (DSPSR_AMD_EINVAL)
 *   out_dev         rows [chan][npol_out] of *nout floats, FPT order like the reference's TimeSeries: any float-aligned address,
 *                   out_pol_stride >= *nout and out_chan_stride >= (npol_out-1)*out_pol_stride + *nout (else DSPSR_AMD_EINVAL,
 *                   nothing launched); only the *nout complete samples of a row are written -- the open one goes to carry_dev
 *   carry_dev       [nchan][npol_out] floats owned by the caller (any content when *carry_count == 0)
 *   carry_count     in: samples already summed into carry_dev (< tscrunch); out: samples left over by this call
 *   nout            out: complete output samples written per row = (carry_in + npart * nkeep) / tscrunch
 * tscrunch = 1 writes the detected samples themselves.  Three-pass and two-pass geometries run it inside the inverse pass; the
 * others (freq_res > 8192, odd factors, matrix response) through an internal detected block + dspsr_amd_tscrunch_fpt -- the same
 * numbers.  Coherence stages four floats per (channel, sample) in the tile the complex samples came from, so it runs inside the
 * inverse pass only where, besides, tscrunch * G <= freq_res with G = ((nkeep + 2 * tscrunch - 2) / tscrunch) | 1 (roughly
 * nfilt_pos + nfilt_neg >= 3 * tscrunch) and freq_res >= 16; elsewhere the object runs perform_detect(COHERENCE, ndim 1) into its
 * own block and dspsr_amd_tscrunch_fpt (npol 4, ndim 1) behind it: the same numbers, *nout and *carry_count.
 * dspsr_amd_filterbank_search_is_fused_state tells which. */
#define DSPSR_AMD_INTENSITY 2
#define DSPSR_AMD_PPQQ 3
int dspsr_amd_filterbank_perform_search(dspsr_amd_filterbank* fb, const float* in_f32_dev, uint64_t in_chan_stride,
                                        uint64_t in_pol_stride, uint64_t in_step, const int8_t* raw_dev, int raw_layout,
                                        float scale, int out_state, uint32_t tscrunch, float* out_dev, uint64_t out_chan_stride,
                                        uint64_t out_pol_stride, float* carry_dev, uint32_t* carry_count, uint64_t npart,
                                        uint64_t* nout);
/* 1: dspsr_amd_filterbank_perform_search runs inside the inverse pass for this object; 0: through the internal detected block */
int dspsr_amd_filterbank_search_is_fused(const dspsr_amd_filterbank* fb);
/* 1: dspsr_amd_filterbank_perform_search(out_state, tscrunch) runs inside the inverse pass for this object; 0: through the internal
 * detected block, and for a null object, an unknown state (Stokes included), tscrunch 0, or a state the object's polarisations do
 * not give.  (dspsr_amd_filterbank_search_is_fused above is this query for PPQQ at a factor of 1, without the polarisation test.) */
int dspsr_amd_filterbank_search_is_fused_state(const dspsr_amd_filterbank* fb, int out_state, uint32_t tscrunch);
/* dsp::TScrunch::fpt_tscrunch (TScrunch.C:148-178; TScrunch::Engine::fpt_tscrunch, dsp/TScrunch.h:61-69, CUDA twin TScrunchCUDA.cu:
 * 204-300: ndim 1 or 2) on device rows [nchan][npol] of ndat_in samples of ndim floats each, every dimension on its own, as a stream:
 * carry / carry_count / nout as above.  Out of place only (digifil scrunches in place on the host, LoadToFil.C:296-304: here every
 * output sample has its own thread). */
int dspsr_amd_tscrunch_fpt(dspsr_amd_ctx* ctx, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                           float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride, uint32_t nchan, uint32_t npol,
                           uint32_t ndim, uint64_t ndat_in, uint32_t sfactor, float* carry_dev /* [nchan][npol][ndim] */,
                           uint32_t* carry_count, uint64_t* nout);
/* dsp::FScrunch::fpt_fscrunch (FScrunch.C:117-145; FScrunch::Engine::fpt_fscrunch, dsp/FScrunch.h:56-64, CUDA twin FScrunchCUDA.cu:
 * 50-90): out row (c, p) = in row (c*sfactor, p); += rows c*sfactor + 1 ... in order.
 * nchan_in must be a multiple of sfactor; out of place only. */
int dspsr_amd_fscrunch_fpt(dspsr_amd_ctx* ctx, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                           float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride, uint32_t nchan_in, uint32_t npol,
                           uint64_t nfloat, uint32_t sfactor);

/* ---- dsp::Detection::Engine (Detection.h:98-106) ------------------------------------------
 * polarimetry(ndim, in, out): in = complex rows [nchan][2][ndat]; in-place allowed for ndim 2
 * (LoadToFold1.C:545-546 uses input==output).  Layouts as above.  Rows at any float-aligned address with any strides (ndim 2 on
 * 16-byte rows, strides that are multiples of 4 floats and an even ndat takes the two-samples-per-thread kernel: the same bits);
 * any nchan and ndat (the kernels walk over more rows and samples than a grid holds). */
int dspsr_amd_detect_polarimetry(dspsr_amd_ctx* ctx, int state, uint32_t ndim, const float* in_dev,
                                 uint64_t in_chan_stride, uint64_t in_pol_stride, float* out_dev,
                                 uint64_t out_chan_stride, uint64_t out_pol_stride, uint32_t nchan, uint64_t ndat);
/* square_law(in,out) (Detection.C:218-320): out[chan][pol][idat] = re^2+im^2 ; intensity!=0 sums the two pols */
int dspsr_amd_detect_square_law(dspsr_amd_ctx* ctx, int intensity, const float* in_dev, uint64_t in_chan_stride,
                                uint64_t in_pol_stride, float* out_dev, uint64_t out_chan_stride,
                                uint64_t out_pol_stride, uint32_t nchan, uint32_t npol, uint64_t ndat);

/* ---- search mode on already channelised 8-bit voltages: `digifil file.dada` with no -F (LoadToFil.C:233-304) ----------------
 * The block is generic DADA: byte ((t * nchan + c) * npol + p) * ndim + d, two's-complement int8, value (float(s) + 0.5f) * scale
 * (BitUnpacker.C:48-80).  raw_dev may be any byte address.
 *
 * dspsr_amd_unpack_fpt replaces dsp::GenericEightBitUnpacker on the device (GenericEightBitUnpackerCUDA.cu:24-83): float FPT rows
 * [nchan][npol] of ndat * ndim floats.  nchan >= 1, npol 1 | 2 | 4, ndim 1 | 2 (so a detected 8-bit file unpacks too).  Rows at any
 * float-aligned address; out_pol_stride >= ndat * ndim and out_chan_stride >= (npol-1)*out_pol_stride + ndat * ndim (else
 * DSPSR_AMD_EINVAL, nothing launched); nothing outside the ndat * ndim floats of a row is written.  ndat = 0: nothing to do. */
int dspsr_amd_unpack_fpt(dspsr_amd_ctx* ctx, const int8_t* raw_dev, float scale, uint32_t nchan, uint32_t npol, uint32_t ndim,
                         uint64_t ndat, float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride);
/* dspsr_amd_unpack_heaps_fpt replaces dsp::MeerKATUnpacker on the device (CUDA::MeerKATUnpackerEngine::unpack,
 * kat/MeerKATUnpackerCUDA.cu): a block of heaps (DSPSR_AMD_RAW_MEERKAT / _SWAP above, raw_layout = DSPSR_AMD_RAW_AT(layout,
 * first_sample)) -> float FPT rows [nchan][npol] of ndat complex samples, stream samples first_sample ... first_sample + ndat - 1
 * of the block.  npol 1 | 2, nchan >= 1; unlike the reference's kernel, ndat need not be a multiple of 256.  raw_dev 16-byte
 * aligned; rows at any float-aligned address, out_pol_stride >= 2 * ndat and out_chan_stride >= (npol-1)*out_pol_stride + 2 * ndat
 * (else DSPSR_AMD_EINVAL, nothing launched); nothing outside the 2 * ndat floats of a row is written.  ndat = 0: nothing to do. */
int dspsr_amd_unpack_heaps_fpt(dspsr_amd_ctx* ctx, const int8_t* raw_dev, int raw_layout, float scale, uint32_t nchan, uint32_t npol,
                               uint64_t ndat, float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride);
/* dspsr_amd_unpack_guppi_fpt replaces dsp::GUPPIUnpacker AND the host un-transpose in front of it (GUPPIBlockFile::load_bytes,
 * guppi/GUPPIBlockFile.C:214-234) on the device: GUPPI / PUPPI raw blocks, as they lie in the file, -> float FPT rows [nchan][npol]
 * of ndat complex samples.  A block's data section is channel-major: run c holds the consecutive samples of channel c, 2 * npol
 * bytes each ((re, im) of polarisation 0, then of polarisation 1, int8); only the first block_nsamp samples of a run are kept (the
 * OVERLAP samples behind them repeat the next block).  raw_dev points at the data section of the block that holds the call's first
 * sample, `first` says where in that block's runs the sample lies.  With u = first + t, stream sample t (0 <= t < ndat) of (chan c,
 * pol p) is read at byte
 *     (u / block_nsamp) * block_stride + c * chan_stride + ((u % block_nsamp) * npol + p) * 2 + d
 * and stored as float(int8) -- no half step and no scale, GUPPIUnpacker.C:74-80, unlike the (int8 + 0.5) * scale of the readers
 * above -- at out_dev[c * out_chan_stride + p * out_pol_stride + 2 t + d].  Nothing outside the 2 * ndat floats of a row is
 * written; nothing outside the kept samples of the runs of the ceil((first + ndat) / block_nsamp) blocks is read.  raw_dev,
 * chan_stride and block_stride are any multiples of one sample (2 * npol bytes): runs that are not 16-byte aligned take narrower
 * loads.  Rows at any float-aligned address (16-byte aligned rows take float4 stores).  ndat = 0: nothing to do.
 * DSPSR_AMD_EINVAL before any launch, the message naming the limit: a null layout; nchan = 0; npol not 1 | 2; block_nsamp = 0;
 * first >= block_nsamp; chan_stride < block_nsamp * 2 * npol; nchan > 1 and block_stride < (nchan - 1) * chan_stride +
 * block_nsamp * 2 * npol; a stride or raw_dev that is not a multiple of 2 * npol; ndat >= 2^60; out_pol_stride < 2 * ndat (npol 2) or
 * out_chan_stride < (npol - 1) * out_pol_stride + 2 * ndat (nchan > 1); a null pointer with ndat > 0. */
typedef struct {
  uint32_t nchan, npol;          /* npol 1 | 2, complex samples */
  uint32_t block_nsamp;          /* kept samples of a run (OVERLAP already taken off) */
  uint32_t first;                /* where the call's first sample lies inside block 0 of raw_dev, < block_nsamp */
  uint64_t chan_stride;          /* bytes from run c to run c+1 of a block  (BLOCSIZE / nchan) */
  uint64_t block_stride;         /* bytes from a block's data section to the next one's */
} dspsr_amd_guppi_layout;
int dspsr_amd_unpack_guppi_fpt(dspsr_amd_ctx* ctx, const int8_t* raw_dev, const dspsr_amd_guppi_layout* layout, uint64_t ndat,
                               float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride);
/* dspsr_amd_unpack_sigproc_fpt replaces dsp::SigProcUnpacker::unpack, OrderFPT branch (sigproc/SigProcUnpacker.C:96-156; the order
 * the reference uses for the format, get_order_supported :23) on the device: the detected spectra of a SIGPROC filterbank file, as
 * they lie in the file, -> float FPT rows [nchan][npol] of ndat floats.  Spectrum t is the S = npol * nchan * nbit / 8 bytes at
 * raw_dev + t * S; value v = ipol * nchan + ichan of it goes to out_dev[ichan * out_chan_stride + ipol * out_pol_stride + t].
 * nbit 8 / 16 / 32: element v as uint8 / uint16 / a float copied bit for bit.  nbit 1 / 2 / 4: byte v * nbit / 8, shifted right by
 * (ichan mod 8 / nbit) * nbit and masked to nbit bits (the lowest bits are the first channel).  The value is float(x) - offset with
 * offset = 127.5 (nbit 8) or 32768 (nbit 16) in the rows ipol > 1 -- the cross products of files dspsr wrote, :101-103 --, else 0:
 * exact in float32.  The `signed` key of the header plays no part, as in the reference.
 * raw_dev at any byte address for nbit <= 8, any 2-byte address for nbit 16, any 4-byte address for nbit 32 (a caller offsets the
 * pointer to the first spectrum of its call, S is often odd): the widest load the address and S allow -- of 16, 8, 4, 2 and 1
 * bytes, at most an eighth of a tile's 16 * nbit bytes -- is chosen once per call.  No byte outside raw_dev ... raw_dev + ndat * S is read.  Rows at any float-aligned address (a row whose
 * address is 16-byte aligned takes float4 stores); nothing outside the ndat floats of a row is written.  ndat = 0: nothing to do.
 * A transpose through LDS in tiles of 64 spectra by 128 values; nbit / 8 bytes read and 4 written per value.
 * DSPSR_AMD_EINVAL before any launch, the message naming the limit: nbit not 1 | 2 | 4 | 8 | 16 | 32; nchan = 0; npol not 1 | 2 | 4;
 * nbit < 8 and nchan * nbit not a multiple of 8 (a polarisation would start inside a byte, where the reference's own addressing
 * goes wrong); raw_dev not a multiple of nbit / 8 bytes (nbit 16, 32); ndat * S > 2^62; out_pol_stride < ndat (npol > 1) or
 * out_chan_stride < (npol - 1) * out_pol_stride + ndat (nchan > 1); a null pointer with ndat > 0. */
int dspsr_amd_unpack_sigproc_fpt(dspsr_amd_ctx* ctx, const void* raw_dev, uint32_t nbit, uint32_t nchan, uint32_t npol, uint64_t ndat,
                                 float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride);
/* ---- two-bit voltages: dsp::TwoBitCorrection on the device (TwoBitCorrection.C, ExcisionUnpacker.C, TwoBitFour.h) -------------
 * One input channel of real samples from npol = 1 | 2 digitisers.  Byte k of the stream belongs to digitiser k % npol and holds four
 * consecutive samples of it, the first in the two most significant bits (ExcisionUnpacker::get_input_offset / get_input_incr,
 * BitTable MostToLeast).  table_type is the code -> (+-lo, +-hi) map of TwoBitTable::generate_unique_values, and with it the two
 * codes that count as low:
 *     code                       0    1    2    3
 *     OFFSET_BINARY            -hi  -lo  +lo  +hi
 *     SIGN_MAGNITUDE           +lo  +hi  -lo  -hi
 *     TWOS_COMPLEMENT          +lo  +hi  -hi  -lo
 * Windows of nsample samples are aligned to the STREAM: raw_dev points at the first byte of the window that holds the call's
 * first sample, first_sample in [0, nsample) says where in that window that sample lies, and the block holds
 * nwindow = ceil((first_sample + ndat) / nsample) whole windows (nwindow * nsample / 4 * npol bytes).  For every (digitiser,
 * window) the low states are counted (n_low); the window's weight is 0 where every byte of it is zero, n_low < nlow_min or
 * n_low > nlow_max (excision_unpack.h:83-85), else 1; its samples become +-lo / +-hi of entry clamp(n_low, nlow_min, nlow_max) -
 * nlow_min of levels_dev (float [nlow_max - nlow_min + 1][2]: lo, hi; dspsr_amd/twobit.py builds it), or 0 where the weight is 0.
 * A digitiser's samples are zeroed for its OWN bad windows only; combining the weights (WeightedTimeSeries::mask_weights) is the
 * caller's.  out_dev: row p at out_dev + p * out_pol_stride receives stream samples first_sample ... first_sample + ndat - 1 of
 * the block; any float-aligned address; nothing outside the ndat floats of a row is written.  weights_dev: uint32 [npol][nwindow];
 * nlow_dev: the same shape, or NULL.  ndat = 0: nothing to do.
 * DSPSR_AMD_EINVAL before any launch, the message naming the limit: nsample not a multiple of 4 in [4, 65536]; nlow_max <= nlow_min
 * or nlow_max > nsample; first_sample >= nsample; npol not 1 | 2; raw_dev not 4-byte aligned; out_pol_stride < ndat with npol 2;
 * an unknown table_type.  dspsr_amd_twobit_check gives the same answers without a device (addresses as integers). */
#define DSPSR_AMD_TWOBIT_OFFSET_BINARY 0
#define DSPSR_AMD_TWOBIT_SIGN_MAGNITUDE 1
#define DSPSR_AMD_TWOBIT_TWOS_COMPLEMENT 2
int dspsr_amd_twobit_check(uint64_t raw_addr, int table_type, uint32_t npol, uint32_t nsample, uint32_t first_sample, uint64_t ndat,
                           uint32_t nlow_min, uint32_t nlow_max, uint64_t out_addr, uint64_t out_pol_stride, char* msg, size_t msg_len);
int dspsr_amd_twobit_unpack(dspsr_amd_ctx* ctx, const uint8_t* raw_dev, int table_type, uint32_t npol, uint32_t nsample,
                            uint32_t first_sample, uint64_t ndat, uint32_t nlow_min, uint32_t nlow_max, const float* levels_dev,
                            float* out_dev, uint64_t out_pol_stride, uint32_t* weights_dev, uint32_t* nlow_dev);
/* dspsr_amd_detect_raw replaces the unpacker, dsp::Detection (DetectionCUDA.cu:180-213 sqld_fpt; Detection.C:218-320 square_law,
 * LoadToFil.C:267-271 Coherence with ndim 1) and dsp::TScrunch (TScrunch.C:148-178) by ONE pass over the block: complex input
 * (ndim 2), npol 1 | 2, any nchan >= 1; the float voltages are never written.  Bit for bit dspsr_amd_unpack_fpt ->
 * dspsr_amd_detect_square_law / dspsr_amd_detect_polarimetry(COHERENCE, ndim 1) -> dspsr_amd_tscrunch_fpt.
 *   out_state       DSPSR_AMD_INTENSITY (npol_out 1) | DSPSR_AMD_PPQQ (2) | DSPSR_AMD_COHERENCE (4 rows: PP, QQ, Re, Im); one input
 *                   polarisation gives Intensity (= PP) only
 *   out_dev, carry_dev [nchan][npol_out], carry_count, nout: the stream contract of dspsr_amd_filterbank_perform_search above, with
 *                   *nout = (carry_in + ndat) / tscrunch; overlapping or too short rows, tscrunch = 0, a null carry_dev or
 *                   carry_count with tscrunch > 1: DSPSR_AMD_EINVAL, nothing launched, *carry_count and *nout as they were.
 *                   tscrunch = 1 needs neither carry_dev nor carry_count.  ndat = 0: nothing to do (*nout = 0).
 * Deterministic: no atomics, the same bits for every split of a stream into calls. */
int dspsr_amd_detect_raw(dspsr_amd_ctx* ctx, const int8_t* raw_dev, float scale, uint32_t nchan, uint32_t npol, uint64_t ndat,
                         int out_state, uint32_t tscrunch, float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride,
                         float* carry_dev, uint32_t* carry_count, uint64_t* nout);

/* ---- search mode (digifil): dsp::TFPFilterbank (TFPFilterbank.C:27-101: forward FFT of 2*nchan real
 * samples per pol and part, Re^2+Im^2 of bins 0..nchan-1, TFP order) + optional pol sum + dsp::TScrunch
 * (TScrunch.C:180-206) fused in one launch.  Real dual-pol 8-bit input, raw_dev = first byte of the block, 2-byte aligned in
 * either byte order (an odd pointer: DSPSR_AMD_EINVAL; a 16-byte aligned block takes the faster whole-range loads).  npart < tscrunch:
 * nothing to do.  Rows of out_dev behind npart/tscrunch - 1 are not written.
 *   out_dev: [npart/tscrunch][nchan][pscrunch ? 1 : 2] floats (PPQQ or Intensity, TimeSeries::OrderTFP) */
typedef struct {
  uint32_t nchan;      /* -F nchan (power of two, 16..8192: both polarisations of one part fill a 2^14-point tile at 8192) */
  uint32_t npol;       /* input polarisations (2) */
  uint32_t pscrunch;   /* 1: Intensity (p0+p1), 0: PPQQ */
  uint32_t tscrunch;   /* -t factor, 0/1 = none */
} dspsr_amd_tfp_config;
int dspsr_amd_tfp_filterbank(dspsr_amd_ctx* ctx, const dspsr_amd_tfp_config* cfg, const int8_t* raw_dev, int raw_layout,
                             float scale, float* out_dev, uint64_t npart);

/* ---- dsp::Fold::Engine (Fold.h:249-312, FoldCUDA.cu) --------------------------------------
 * The engine owns the device-resident profile (get_profiles()).  Call order per Fold::fold
 * (Fold.C:724-829): set_nbin, set_ndat, set_bin x ndat (or set_bins), fold.  synch copies to host. */
int dspsr_amd_fold_create(dspsr_amd_ctx* ctx, dspsr_amd_fold** fold);
void dspsr_amd_fold_destroy(dspsr_amd_fold* fold);
/* shape of the input TimeSeries / output PhaseSeries (Fold::Engine::setup, Fold.C:973-1007): ndim 1, 2 or 4 with any npol, or
 * ndim 14 with npol 1 and only with it -- the fourth moments of the Stokes parameters, below; same rule in bind_profile */
int dspsr_amd_fold_set_shape(dspsr_amd_fold* fold, uint32_t nchan, uint32_t npol, uint32_t ndim, uint32_t nbin);
/* Fold::Engine::setup (Fold.C:968-1011): fold INTO the engine-owned device PhaseSeries -- profile_dev =
 * get_profiles()->get_datptr(0,0), span_floats = get_nfloat_span() (floats between consecutive (chan, pol) rows, each
 * row nbin*ndim floats) -- so that Fold::prepare_output / zero / mixable (Fold.C:88-94,123-148,495-508), which act on
 * get_profiles(), see the sums.  The buffer stays the caller's; profile_dev = NULL returns to a library-owned profile. */
int dspsr_amd_fold_bind_profile(dspsr_amd_fold* fold, float* profile_dev, uint64_t span_floats, uint32_t nchan,
                                uint32_t npol, uint32_t ndim, uint32_t nbin);
int dspsr_amd_fold_set_nbin(dspsr_amd_fold* fold, uint32_t nbin);                        /* FoldCUDA.cu:64-70 */
int dspsr_amd_fold_set_ndat(dspsr_amd_fold* fold, uint64_t ndat, uint64_t idat_start);   /* FoldCUDA.cu:72-82 */
int dspsr_amd_fold_set_bin(dspsr_amd_fold* fold, uint64_t idat, double ibin, double bins_per_sample); /* :84-113 */
/* whole plan at once: the double recurrence of Fold.C:744-787 run inside the library;
 * hits_host[nbin] (may be NULL) is incremented like Fold.C:783; returns ndat folded via *ndat_folded.
 * Call order: set_nbin, set_ndat, then set_bin / set_bins (several calls may build one plan: a run left open by one call
 * goes on in the next), then fold.  A fold (or a fused fold) uses the plan up; a plan built after it without a new set_nbin
 * opens a fresh run at its first sample, so every sample counted in hits_host and ndat_folded is folded by the next fold. */
int dspsr_amd_fold_set_bins(dspsr_amd_fold* fold, double phi, double phase_per_sample, uint64_t ndat,
                            uint64_t idat_start, uint32_t* hits_host, uint64_t* ndat_folded);
/* the same with the weights of the input (Fold.C:686-716,746-763: WeightedTimeSeries, one weight per ndatperweight samples,
 * sample idat belongs to weight (idat + weight_idat) / ndatperweight): samples of a zero weight are left out of the plan,
 * of hits[] and of *ndat_folded.  The hook for flagged / dropped data; spectral kurtosis itself is dspsr_amd_sk below. */
int dspsr_amd_fold_set_bins_weighted(dspsr_amd_fold* fold, double phi, double phase_per_sample, uint64_t ndat,
                                     uint64_t idat_start, const uint32_t* weights_host, uint64_t nweights,
                                     uint64_t ndatperweight, uint64_t weight_idat, uint32_t* hits_host,
                                     uint64_t* ndat_folded);
/* fold(): accumulate in_dev rows (get_datptr(ichan,ipol) = in_dev + ichan*in_chan_stride + ipol*in_pol_stride)
 * into the device profile using the plan built since the last set_nbin (FoldCUDA.cu:586-697) */
int dspsr_amd_fold_fold(dspsr_amd_fold* fold, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride);
/* Fold::Engine::fold of several Folds whose input is the SAME detected TimeSeries (LoadToFold1.C:939-960: one Fold per
 * pulsar).  Every fold must have its plan set (set_nbin / set_ndat / set_bins[_weighted]) and share ctx, nchan, npol, ndim;
 * nbin and the plan may differ.  Each profile ends bit-identical to dspsr_amd_fold_fold(folds[k], ...) alone.
 * Two or more exact-order plans of the chunk kernels share launches of at most DSPSR_AMD_FOLD_MANY_MAX plans (sizes balanced),
 * each of which reads the detected rows once; *nshared (may be NULL): how many folds took a shared launch (0 when only one plan
 * is exact-order); the others (a lone exact-order plan, LONG runs, unaligned rows, nbin beyond the chunk kernels, empty plans)
 * were folded one by one inside this call.  NULL entries, a fold given twice, or folds
 * of different contexts or shapes: DSPSR_AMD_EINVAL before any plan is used.  nfold == 0: nothing to do. */
#define DSPSR_AMD_FOLD_MANY_MAX 8
int dspsr_amd_fold_fold_many(dspsr_amd_fold* const* folds, uint32_t nfold, const float* in_dev,
                             uint64_t in_chan_stride, uint64_t in_pol_stride, uint32_t* nshared);
/* fold() of an input that carries zeroed (RFI-excised) samples -- Fold::Engine::zeroed_samples with hits_nchan == nchan
 * (Fold.C:853-866, fold1bin*hits FoldCUDA.cu:415-576,622): as dspsr_amd_fold_fold, and hits_dev[ichan*nbin + ibin] (device,
 * uint32) is incremented by the number of planned samples of polarisation 0 whose first float is not zero.  The hook the
 * reference's spectral-kurtosis chain needs; the excision itself is dspsr_amd_sk below. */
int dspsr_amd_fold_fold_zeroed(dspsr_amd_fold* fold, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                               uint32_t* hits_dev);
float* dspsr_amd_fold_profiles_dev(dspsr_amd_fold* fold);   /* device [nchan][npol][nbin][ndim] (get_profiles) */
uint64_t dspsr_amd_fold_get_ndat_folded(const dspsr_amd_fold* fold);
int dspsr_amd_fold_zero(dspsr_amd_fold* fold);                                            /* Engine::zero */
int dspsr_amd_fold_synch(dspsr_amd_fold* fold, float* profile_host);                      /* FoldCUDA.cu:127-152 (blocks) */

/* ---- fourth-order moments of the Stokes parameters, `dspsr -4` (LoadToFold1.C:552-568; detection forced to Stokes, ndim 4:
 * :1119-1123) ----
 * dsp::FourthMoment::transformation (Signal/General/FourthMoment.C:29-77): per channel and sample the four Stokes floats, copied
 * bit for bit, then in[i] * in[j] for i <= j in the loop order of :67-72 (00 01 02 03 11 12 13 22 23 33), each one float multiply
 * rounded to nearest: rows of ndat*4 floats `in_chan_stride` apart in, rows of ndat*14 floats `out_chan_stride` apart out (npol
 * 1, ndim 14, state FourthMoment: :39-42).  Out of place only, as in the reference (:25).  DSPSR_AMD_EINVAL before any launch:
 * in_dev == out_dev; input rows not 16-byte aligned (in_dev, in_chan_stride % 4) or output rows not 8-byte aligned (out_dev,
 * out_chan_stride % 2); a stride shorter than its row (ndat*4, ndat*14); nchan > 65535.  ndat == 0: nothing to do (:49-50). */
int dspsr_amd_fourth_moment(dspsr_amd_ctx* ctx, const float* in_dev, uint64_t in_chan_stride, float* out_dev,
                            uint64_t out_chan_stride, uint32_t nchan, uint64_t ndat);
/* Folding the moments (Fold.C:835-891 is a plain sum over whatever ndim arrives; Archiver.C:382-405 takes npol*ndim == 14): a
 * fold of shape npol 1 x ndim 14.  set_nbin, set_ndat, set_bin, set_bins[_weighted], zero, synch, profiles_dev and
 * get_ndat_folded work on it as on any shape.  dspsr_amd_fold_fold reads ndim 14 rows, the output of dspsr_amd_fourth_moment
 * (in_pol_stride is not used: one polarisation).  dspsr_amd_fold_fold_moments reads the ndim 4 Stokes rows themselves (npol 1)
 * and forms the ten products in registers, so the 14-float stream is never written or read; DSPSR_AMD_EINVAL on a fold of any
 * other shape.  The two are bit-identical on the same Stokes samples, plan and device: one accumulation, two loaders
 * (csrc/fold_moments.hip).  Sums as for every fold: no atomics, the same bits run to run; plans of runs shorter than 64 samples
 * in strict time order (Fold.C:844-852), plans with a longer run re-associated like the long-run fold, deterministically.
 * Rows at any float-aligned address (16-byte aligned rows load faster).  dspsr_amd_fold_fold_many and
 * dspsr_amd_fold_fold_zeroed refuse a 14-shape (DSPSR_AMD_EINVAL), and the fused filterbank+fold entry points stay npol 1 x
 * ndim 4 / npol 2 x ndim 2: `-4` runs perform_detect (Stokes, ndim 4), then fold_moments. */
int dspsr_amd_fold_fold_moments(dspsr_amd_fold* fold, const float* stokes_dev, uint64_t in_chan_stride);

/* ---- dsp::CyclicFoldEngine: cyclic spectra, `dspsr -cyclic N [-cyclicoversample M]` (LoadToFold1.C:534-539,999-1044) ----------
 * Lag-domain folding of the filterbank's complex voltages (Analytic float rows in FPT order: what
 * dspsr_amd_filterbank_perform[_raw] writes).  The semantics are those of the reference's CPU engine, dsp::CyclicFoldEngine
 * (Signal/Pulsar/CyclicFold.C); its CUDA engine follows a rounded plan (CyclicFoldEngineCUDA.cu:232-331) that differs from the
 * CPU engine's per-sample plan, and where the two disagree the CPU engine is the definition here.
 *   sizes   nlag = mover * nchan_cyclic / 2 + 1 (dsp/CyclicFold.h:66); nchan_spec = 2 nlag - 2; nchan_spec / mover output
 *           channels per input channel, ndim 1; npol_out 1 (Intensity; PP for one input polarisation), 2 (PPQQ) or 4
 *           (Coherence) (CyclicFold.C:96-119); one input polarisation allows npol_out = 1 only.
 *   plan    set_bin (CyclicFold.C:293-301): plan0[i] = unsigned(ibin), plan1[i] = unsigned(ibin + 0.5 bins_per_sample) % nbin,
 *           i = idat - idat_start; set_bins runs the double recurrence of Fold.C:744-787 (as dspsr_amd_fold_binplan) inside the
 *           library, hits_host[] and *ndat_folded count EVERY sample of the call (Fold.C:783-784), the last nlag ones included.
 *   fold    (CyclicFold.C:339-448) ndat_fold <= nlag: nothing is accumulated.  Else for idat < ndat_fold - nlag, ilag < nlag:
 *             lag[bin][pol][chan][ilag] += x[idat] * conj(y[idat + ilag]),  bin = plan[ilag % 2][idat + ilag / 2]
 *           (re += a.re b.re + a.im b.im, im += a.im b.re - a.re b.im; :316-321), (x, y) = (p0,p0) + (p1,p1) into one sum for
 *           npol_out 1; (p0,p0), (p1,p1) for 2; then (p0,p1), (p1,p0) for 4.  Products that would span two calls are dropped, as in
 *           the reference.  Rows: in_dev + chan * in_chan_stride + pol * in_pol_stride + 2 * idat_start (strides in floats, any
 *           stride >= the row, rows 8-byte aligned: else DSPSR_AMD_EINVAL before a launch).  Input is only read.
 * Sums are float, re-associated (per run of a bin and per time segment; the cut depends on the shape alone) and use fused
 * multiply-adds: no atomics, the same bits run to run and for the same sequence of fold calls.
 * set_shape allocates the device lag array, nbin * npol_out * nchan * nlag * 2 floats, zeroed (and, for shapes with few
 * (channel, lag) owners, up to 64 partial arrays of that size within 2 GiB): DSPSR_AMD_ENOMEM if it does not fit.  nlag in
 * [2, 65536], nchan <= 65535, ndat < 2^31 per call; anything else DSPSR_AMD_EINVAL before a launch.
 * Call order per Fold::fold (Fold.C:724-829): set_ndat, set_bin x ndat (or set_bins), fold.
 * A set_shape that changes any of nchan, npol_in, npol_out, nlag, mover, nbin starts from zero AND drops the block and its plan
 * (they hold bins of the old nbin): set_ndat must follow it before set_bin, set_bins or fold -- until then fold returns
 * DSPSR_AMD_ESTATE, launches nothing and leaves the lag data as they are.  set_shape with the values it already has keeps the
 * sums, the block and the plan. */
int dspsr_amd_cyclic_fold_create(dspsr_amd_ctx* ctx, dspsr_amd_cyclic_fold** fold);
void dspsr_amd_cyclic_fold_destroy(dspsr_amd_cyclic_fold* fold);
int dspsr_amd_cyclic_fold_set_shape(dspsr_amd_cyclic_fold* fold, uint32_t nchan, uint32_t npol_in, uint32_t npol_out,
                                    uint32_t nlag, uint32_t mover, uint32_t nbin);
int dspsr_amd_cyclic_fold_set_ndat(dspsr_amd_cyclic_fold* fold, uint64_t ndat, uint64_t idat_start);   /* CyclicFold.C:234-256 */
int dspsr_amd_cyclic_fold_set_bin(dspsr_amd_cyclic_fold* fold, uint64_t idat, double ibin, double bins_per_sample);
int dspsr_amd_cyclic_fold_set_bins(dspsr_amd_cyclic_fold* fold, double phi, double phase_per_sample, uint64_t ndat,
                                   uint64_t idat_start, uint32_t* hits_host, uint64_t* ndat_folded);
int dspsr_amd_cyclic_fold_fold(dspsr_amd_cyclic_fold* fold, const float* in_dev, uint64_t in_chan_stride,
                               uint64_t in_pol_stride);
int dspsr_amd_cyclic_fold_zero(dspsr_amd_cyclic_fold* fold);                               /* CyclicFold.C:283-291 */
/* device lag array [bin][pol][chan][lag][re, im] (get_lagdata_ptr, CyclicFold.C:329-337), valid in stream order */
float* dspsr_amd_cyclic_fold_lagdata_dev(dspsr_amd_cyclic_fold* fold);
/* copy to the host in the same order and wait (CyclicFoldEngineCUDA.cu:72-107): a C++ caller hands it to
 * dsp::CyclicFoldEngine::synch, any other to dspsr_amd_cyclic_lags_to_spectra */
int dspsr_amd_cyclic_fold_synch_lags(dspsr_amd_cyclic_fold* fold, float* lagdata_host);

/* ---- dsp::PhaseLockedFilterbank: pulse-phase-resolved spectra, `dspsr -G nbin` (LoadToFold1.C:386-456) ---------------------
 * Replaces the loop body of Signal/Pulsar/PhaseLockedFilterbank.C:254-297 (the reference has a CPU implementation only).  The
 * caller walks its own bin_divider (:208-235) and hands every accepted division over as a WINDOW (idat_start, bin), in time order.
 *   input   float rows as the filterbank and dspsr_amd_unpack_fpt write them: element (chan, pol, t) at
 *           in_dev + chan * chan_stride + pol * pol_stride + t * ndim_in floats; ndim_in 2 = Analytic, 1 = Nyquist (:100-110);
 *           ndat samples per row.  Analytic rows 8-byte aligned (pointer, even strides), Nyquist rows float aligned.
 *   window  ndat_fft = nchan (Analytic) or 2 nchan (Nyquist) samples from idat_start; X_p[k] = sum_n x_p[idat_start + n]
 *           exp(-2 pi i k n / ndat_fft), k < nchan, unnormalised (fcc1d / bins 0 .. nchan-1 of frc1d, :263-266; the Nyquist
 *           form is one nchan-point complex transform of the packed pairs plus the Hermitian split).
 *   output  profile [nchan_in * nchan][npol_out][nbin] floats, channel chan * nchan + k in raw transform order, DC first (the
 *           reference records nsub_swap = nchan_in instead of reordering, :149,159).  npol_out 1: += |X_0|^2 + |X_1|^2 over the
 *           input polarisations present; 2: plane p += |X_p|^2; 4: also plane 2 += re0 re1 + im0 im1, plane 3 += re0 im1 - im0 re1
 *           (:269-295).
 *   limits  nchan a power of two in [2, 8192] (the reference takes any length); nchan < 2 && nbin < 2 refused (:61-63);
 *           npol_out in {1, 2, 4} (:44-46); npol_in 1 allows npol_out 1 only (:138-141); nchan_in <= 65535; ndat and nwin
 *           < 2^31 per call; every window inside the rows (idat_start + ndat_fft <= ndat), bin < nbin, idat_start
 *           non-decreasing.  Anything else: DSPSR_AMD_EINVAL with a message, nothing launched.
 * Sums are float and deterministic, without atomics: the windows of a call are grouped by bin and cut into segments (the cut
 * depends on the call's arguments alone); the windows of a bin are added in time order within a segment, segments in segment
 * order, and every profile element has one owner per launch.  Bins without a window in a call are not written.  The profile
 * accumulates over calls until dspsr_amd_plfb_zero; set_shape with a new shape allocates (DSPSR_AMD_ENOMEM) and zeroes, with the
 * values it already has it keeps the sums.
 * The two check functions are the refusals alone, on the host, with the message in msg (no device, no context): set_shape and
 * accumulate call them first. */
int dspsr_amd_plfb_check_shape(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t nchan, uint32_t npol_out,
                               uint32_t nbin, char* msg, size_t msg_len);
int dspsr_amd_plfb_check_windows(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t nchan, uint32_t nbin,
                                 uint64_t in_addr, uint64_t chan_stride, uint64_t pol_stride, uint64_t ndat, uint64_t nwin,
                                 const uint64_t* idat_start_host, const uint32_t* bin_host, char* msg, size_t msg_len);
int dspsr_amd_plfb_create(dspsr_amd_ctx* ctx, dspsr_amd_plfb** plfb);
void dspsr_amd_plfb_destroy(dspsr_amd_plfb* plfb);
int dspsr_amd_plfb_set_shape(dspsr_amd_plfb* plfb, uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t nchan,
                             uint32_t npol_out, uint32_t nbin);
int dspsr_amd_plfb_accumulate(dspsr_amd_plfb* plfb, const float* in_dev, uint64_t chan_stride, uint64_t pol_stride, uint64_t ndat,
                              uint64_t nwin, const uint64_t* idat_start_host, const uint32_t* bin_host);
int dspsr_amd_plfb_zero(dspsr_amd_plfb* plfb);                                             /* PhaseLockedFilterbank.C:151-152 */
/* device profile [nchan_in * nchan][npol_out][nbin], valid in stream order */
float* dspsr_amd_plfb_profile_dev(dspsr_amd_plfb* plfb);
/* copy it to the host and wait */
int dspsr_amd_plfb_synch(dspsr_amd_plfb* plfb, float* profile_host);

/* ---- passband integration: dsp::Bandpass on the device (Signal/General/Bandpass.C:50-175) ---------------------------------
 * The operator behind dspsr -R (dsp::RFIFilter integrates one second of undetected input through it, RFIFilter.C:76-95) and
 * the reference's passband tool.  Per input channel the ndat samples of a call are cut into npart = ndat / nsamp_fft whole,
 * contiguous transforms (nsamp_fft = 2 * resolution real samples, ndim_in 1, or resolution complex samples, ndim_in 2); trailing
 * samples that do not fill a transform are not read.  Forward, unnormalised; Nyquist input keeps bins 0 .. resolution-1 of the
 * real-to-complex transform.  pass[npol_out][nchan_in][resolution] +=  re*re + im*im per polarisation (npol_out = npol_in,
 * Response.C:456-492), or PP, QQ, Re P*Q, Im P*Q (npol_out = 4 with npol_in = 2, cross_detect_int, Response.C:587-612).
 * resolution: a power of two in [2, 8192]; nchan_in <= 65535 and nchan_in * resolution <= 2^24 (the per-segment sums of a launch,
 * counted for four output polarisations, stay within 256 MiB).  Not built, refused by name: apodization, Bandpass::set_response, detected input.
 * Every refusal is DSPSR_AMD_EINVAL with the limit's name (dspsr_amd_last_error) before any launch or allocation.
 *   accumulate     : float rows, element (chan, pol, t) = in + chan*chan_stride + pol*pol_stride + t*ndim_in; any float-aligned
 *                    address, strides >= the row
 *   accumulate_raw : the 8-bit block, DSPSR_AMD_RAW_GENERIC (any nchan_in / npol_in / ndim_in) or DSPSR_AMD_RAW_CASPSR (one channel,
 *                    two real polarisations, block on an 8-byte group); value = (int8 + 0.5) * scale; DSPSR_AMD_RAW_UWB16 is refused
 *   zero           : Bandpass::reset_output -- the passband and the integration length
 *   synch          : the passband on the host (waits) and the samples integrated per row so far, npart * nsamp_fft summed over
 *                    the calls (Bandpass.C:164: integration_length = that / rate)
 * The same sequence of calls gives the same bits (no atomics; the work is cut by (npart, nchan_in, resolution) alone).
 * check_shape / check_input: the device-free halves of set_shape / accumulate (raw_layout < 0: float rows); check_input also
 * returns the launch arithmetic: parts per workgroup tile, tiles per segment, segments. */
typedef struct dspsr_amd_bandpass dspsr_amd_bandpass;
int dspsr_amd_bandpass_check_shape(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t resolution, uint32_t npol_out,
                                   char* msg, size_t msg_len);
int dspsr_amd_bandpass_check_input(uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t resolution, int raw_layout,
                                   uint64_t in_addr, uint64_t chan_stride, uint64_t pol_stride, uint64_t ndat,
                                   uint32_t* parts_per_tile, uint32_t* tiles_per_segment, uint32_t* nsegment, char* msg,
                                   size_t msg_len);
int dspsr_amd_bandpass_create(dspsr_amd_ctx* ctx, dspsr_amd_bandpass** out);
void dspsr_amd_bandpass_destroy(dspsr_amd_bandpass* bp);
int dspsr_amd_bandpass_set_shape(dspsr_amd_bandpass* bp, uint32_t nchan_in, uint32_t npol_in, uint32_t ndim_in, uint32_t resolution,
                                 uint32_t npol_out);
int dspsr_amd_bandpass_accumulate(dspsr_amd_bandpass* bp, const float* in_dev, uint64_t chan_stride, uint64_t pol_stride,
                                  uint64_t ndat);
int dspsr_amd_bandpass_accumulate_raw(dspsr_amd_bandpass* bp, const void* raw_dev, int raw_layout, float scale, uint64_t ndat);
int dspsr_amd_bandpass_zero(dspsr_amd_bandpass* bp);
/* device passband [npol_out][nchan_in][resolution], valid in stream order */
float* dspsr_amd_bandpass_pass_dev(dspsr_amd_bandpass* bp);
int dspsr_amd_bandpass_synch(dspsr_amd_bandpass* bp, float* pass_host, double* integration_samples);

/* ---- dsp::SpectralKurtosis (dspsr -skz): estimate, detect, mask ---------------------------------------------------------
 * Reference: Signal/General/SpectralKurtosis.C, LoadToFold1.C:458-532.  The CPU branch in FPT order is the definition (where the
 * reference's CUDA engines differ from it, it wins).  Input: complex rows [nchan][npol][ndat], ndim 2, element (chan, pol, t) =
 * in + chan*chan_stride + pol*pol_stride + 2*t (strides in floats).  npart = ndat / M; the ndat % M samples behind are not touched.
 *   sk_limits   : host only.  dsp::SKLimits(M, std_devs) rounded to float (SKLimits.C, PearsonIV.C; SpectralKurtosis.C:390-391).
 *                 M >= 32768: 1 -+ std_devs*sqrt(4/M).  Where the reference's Newton iteration gives up, the limit is its starting
 *                 guess, the same expression.  M < 32 (the Pearson IV parameters are not finite below 24) or std_devs == 0: EINVAL.
 *   set_shape   : M in [32, 65536], npol 1 or 2, nchan in [1, 65535].  A new shape zeroes the counters.
 *   set_options : std_devs (> 0); the channel range [chan_start, chan_end) of tscr, fscr and the counters, chan_end == 0: nchan;
 *                 the three detections can be disabled (SpectralKurtosis::set_options).  Needs a shape.
 *   compute     : (:302-371) per (part, chan, pol) S1 = sum |x|^2, S2 = sum |x|^4 in float, one rounding per operation (no fused
 *                 multiply-add); estimates[(part*nchan + chan)*npol + pol] = M_fac * (M * (S2 / (S1*S1)) - 1), 0 when S1 == 0,
 *                 M_fac = (M+1)/(M-1) in unsigned integers (:253); unless tscr is disabled estimates_tscr[chan*npol + pol] from the
 *                 per-part sums added in part order, M_t = float(M*npart), factor (M_t+1)/(M_t-1) in float.  The sums over the M
 *                 samples of one part run in a fixed tree that depends on M alone (csrc/sk.hip: k_sk_compute); no atomics: the same
 *                 bits for any npart, launch shape or cut of a stream into calls.  ndat < M: nothing to do.
 *   reset_mask, detect_tscr, detect_skfb, detect_fscr, count_zapped : the steps of SpectralKurtosis::detect (:413-454) as its Engine
 *                 interface cuts them, on the estimates of the last compute; comparisons are V > upper || V < lower.
 *                 detect_tscr: a channel of the range with any polarisation outside the limits is zapped in all parts.
 *                 detect_skfb: any polarisation outside zaps (part, chan), all channels; counted where chan_start < chan < chan_end.
 *                 detect_fscr (:684-741): per part and polarisation the sequential float sum, in channel order, of the channels of
 *                 the range not yet zapped, divided by their count cnt; one_sigma = sqrt(mu2 / float(cnt)), mu2 =
 *                 4M^2/((M-1)(M+2)(M+3)) in float; outside 1 -+ (1+std_devs)*one_sigma in either polarisation zaps all channels.
 *                 count_zapped (:605-665): zap_counts[0], filtered / unfiltered sums (float, part order) and hits over the range;
 *                 also npart_total += npart*nchan (:434) and unfiltered_hits += npart.
 *   mask        : (:747-797) out = zapmask[part*nchan + chan] ? 0 : in for both polarisations over npart*M samples.  out == in
 *                 (same strides) writes zeros over the zapped parts only and reads no sample.  The output carries zeroed data:
 *                 fold it with dspsr_amd_fold_fold_zeroed.
 *   transform   : compute, reset_mask, detect_tscr, detect_skfb, detect_fscr (each unless disabled), count_zapped, mask, with the
 *                 limits of sk_limits for M and, cached per distinct M*npart, for the tscr estimate (:476-501).
 *   get_statistics : waits.  counts[6] = zap_counts[all, skfb, fscr, tscr], npart_total, unfiltered_hits; filtered_hits[nchan];
 *                 filtered_sum / unfiltered_sum[nchan*npol].  Any pointer may be NULL.  reset_count zeroes them all.
 * Refused with DSPSR_AMD_EINVAL and the limit's name before any launch: a shape outside the limits above, ndat >= 2^31, rows not
 * 8-byte aligned, strides shorter than the row, rows that overlap one another, input and output that partly overlap,
 * std_devs == 0, chan_start >= chan_end, chan_end > nchan. */
typedef struct dspsr_amd_sk dspsr_amd_sk;
int dspsr_amd_sk_limits(uint32_t M, uint32_t std_devs, float* lower, float* upper);
int dspsr_amd_sk_create(dspsr_amd_ctx* ctx, dspsr_amd_sk** out);
void dspsr_amd_sk_destroy(dspsr_amd_sk* sk);
int dspsr_amd_sk_set_shape(dspsr_amd_sk* sk, uint32_t nchan, uint32_t npol, uint32_t M);
int dspsr_amd_sk_set_options(dspsr_amd_sk* sk, uint32_t std_devs, uint32_t chan_start, uint32_t chan_end, int no_fscr, int no_tscr,
                             int no_ft);
int dspsr_amd_sk_compute(dspsr_amd_sk* sk, const float* in_dev, uint64_t chan_stride, uint64_t pol_stride, uint64_t ndat);
int dspsr_amd_sk_reset_mask(dspsr_amd_sk* sk);
int dspsr_amd_sk_detect_tscr(dspsr_amd_sk* sk, float lower, float upper);
int dspsr_amd_sk_detect_skfb(dspsr_amd_sk* sk, float lower, float upper);
int dspsr_amd_sk_detect_fscr(dspsr_amd_sk* sk);
int dspsr_amd_sk_count_zapped(dspsr_amd_sk* sk);
int dspsr_amd_sk_mask(dspsr_amd_sk* sk, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride, float* out_dev,
                      uint64_t out_chan_stride, uint64_t out_pol_stride);
int dspsr_amd_sk_transform(dspsr_amd_sk* sk, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride, float* out_dev,
                           uint64_t out_chan_stride, uint64_t out_pol_stride, uint64_t ndat);
/* of the last compute, valid in stream order: parts, estimates [npart][nchan][npol], estimates_tscr [nchan][npol], zapmask [npart][nchan] */
uint64_t dspsr_amd_sk_npart(dspsr_amd_sk* sk);
float* dspsr_amd_sk_estimates_dev(dspsr_amd_sk* sk);
float* dspsr_amd_sk_estimates_tscr_dev(dspsr_amd_sk* sk);
uint8_t* dspsr_amd_sk_zapmask_dev(dspsr_amd_sk* sk);
int dspsr_amd_sk_get_statistics(dspsr_amd_sk* sk, uint64_t* counts, uint64_t* filtered_hits, float* filtered_sum, float* unfiltered_sum);
int dspsr_amd_sk_reset_count(dspsr_amd_sk* sk);

/* ---- the sub-integration dump over RCCL / xGMI: the ONE exchange of the path -----------------------------------------
 * Reference hook: dsp::Subint<Fold>::transformation emits the finished sub-integration (Signal/Pulsar/dsp/Subint.h:291-303);
 * merging semantics = PhaseSeries::combine (Signal/Pulsar/PhaseSeries.C:442-484); the reference merges its threads' pieces
 * on the host today (Signal/General/MultiThread.C:274-379).  One process per GPU, one communicator per pipeline context.
 *   dspsr_amd_comm_unique_id : ncclGetUniqueId -- rank 0 calls it and hands the 128 bytes to every rank by any host means
 *                              (MPI, a file, a socket; dspsr's own MPI transport, Kernel/Classes/mpi)
 *   dspsr_amd_comm_create    : ncclCommInitRank on the context's device (collective: every rank calls it)
 *   dspsr_amd_reduce_profiles_start : snapshot of this rank's device profile rows (`nrow` rows of `row_floats` floats,
 *       `span_floats` apart -- Fold::Engine::get_profiles()) on the context's stream, then ONE collective on the
 *       communicator's own stream, so the caller may zero the profile and launch the next block at once:
 *         DSPSR_AMD_REDUCE_SUM    time-slice replicas: profile, hits[], ndat_total and integration_length all SUMMED onto
 *                                 `root` in one packed ncclReduce
 *         DSPSR_AMD_REDUCE_GATHER sub-band shards (rank g = input channel g): the ranks' slices delivered to `root` in rank
 *                                 order (ncclGather); hits[] / lengths are identical on every rank and are the root's own.
 *                                 check_hits != 0 adds a MIN/MAX all-reduce of hits[] to the same group.
 *   dspsr_amd_reduce_profiles_finish : waits for the exchange.  On `root`: profile_host receives nrow*row_floats floats
 *       (SUM) or nranks*nrow*row_floats floats (GATHER), packed; hits_host[nbin], *integration_length, *ndat_total the
 *       merged values.  Other ranks receive nothing.  *hits_identical (every rank; may be NULL) = 0 if check_hits found
 *       ranks that disagree. */
typedef struct dspsr_amd_comm dspsr_amd_comm;
#define DSPSR_AMD_UNIQUE_ID_BYTES 128
#define DSPSR_AMD_REDUCE_SUM 0
#define DSPSR_AMD_REDUCE_GATHER 1
/* optional, before the first communicator: the RCCL shared object to open (default: librccl.so.1 from the loader path,
 * then /opt/rocm/lib).  A host process that carries its own ROCm runtime (PyTorch) names the RCCL built against it. */
int dspsr_amd_comm_set_library(const char* path);
int dspsr_amd_comm_unique_id(void* id_out);
int dspsr_amd_comm_create(dspsr_amd_ctx* ctx, int nranks, int rank, const void* unique_id, dspsr_amd_comm** comm);
void dspsr_amd_comm_destroy(dspsr_amd_comm* comm);
int dspsr_amd_comm_rank(const dspsr_amd_comm* comm);
int dspsr_amd_comm_size(const dspsr_amd_comm* comm);
int dspsr_amd_reduce_profiles_start(dspsr_amd_comm* comm, int mode, int root, const float* profile_dev, uint64_t span_floats,
                                    uint64_t nrow, uint64_t row_floats, const uint32_t* hits_host, uint32_t nbin,
                                    double integration_length, uint64_t ndat_total, int check_hits);
int dspsr_amd_reduce_profiles_finish(dspsr_amd_comm* comm, float* profile_host, uint32_t* hits_host, double* integration_length,
                                     uint64_t* ndat_total, int* hits_identical);
/* root, after finish: the merged profile where the exchange left it -- the communicator's pinned host buffer (*nfloat floats,
 * valid until the next start) -- for a writer that wants to read it in place (pass profile_host = NULL to finish) */
const float* dspsr_amd_reduce_profiles_result(const dspsr_amd_comm* comm, uint64_t* nfloat);

/* ---- integer-sample inter-channel delay (-K): dsp::SampleDelay (Signal/General/SampleDelay.C:52-195) --------------
 * create    : SampleDelay::build (:52-102) from the delay of each row, delays_host[ichan*npol+ipol] (the values
 *             SampleDelayFunction::get_delay returns); absolute = function->get_absolute()
 * transform : SampleDelay::transformation (:123-195): out row i = in row shifted by its applied delay, ndat_out =
 *             ndat_in - total_delay (0 if negative); in == out allowed (LoadToFold1.C:617-618); strides in floats.
 *             The caller shifts the start time by zero_delay samples (:159) and re-presents the last total_delay
 *             samples with the next block (InputBuffering, :117,146). */
typedef struct dspsr_amd_sample_delay dspsr_amd_sample_delay;
int dspsr_amd_sample_delay_create(dspsr_amd_ctx* ctx, uint32_t nchan, uint32_t npol, const int64_t* delays_host,
                                  int absolute, dspsr_amd_sample_delay** out);
void dspsr_amd_sample_delay_destroy(dspsr_amd_sample_delay* h);
int64_t dspsr_amd_sample_delay_zero_delay(const dspsr_amd_sample_delay* h);
uint64_t dspsr_amd_sample_delay_total_delay(const dspsr_amd_sample_delay* h);
int dspsr_amd_sample_delay_transform(dspsr_amd_sample_delay* h, const float* in_dev, uint64_t in_chan_stride,
                                     uint64_t in_pol_stride, float* out_dev, uint64_t out_chan_stride,
                                     uint64_t out_pol_stride, uint32_t ndim, uint64_t ndat_in, uint64_t* ndat_out);

/* ---- search-mode output stage: dsp::Rescale + dsp::SigProcDigitizer on TFP-ordered data ----------
 * dspsr_amd_rescale_*        : dsp::Rescale (Signal/General/Rescale.C:157-420), scalar offset/scale per (pol, chan)
 *                              re-estimated every `interval_samples` samples (0 = length of the first block) and once
 *                              right after the first call; `constant` keeps the first estimate (set_constant, :50).
 *                              in == out is allowed (digifil rescales in place, LoadToFil.C:325-326).
 * dspsr_amd_sigproc_digitize : dsp::SigProcDigitizer::pack, TFP branch (Kernel/Formats/sigproc/SigProcDigitizer.C:80-236)
 *                              nbit 1/2/4/8/16 or -32 (pack_float :309-342); flip_band = input bandwidth > 0,
 *                              swap_band = input->get_swap() (ChannelSort :38-66); input_scale = input->get_scale().
 * dspsr_amd_pscrunch_tfp     : dsp::PScrunch, TFP branch (Signal/General/PScrunch.C:36-90): (p0 + p1) * float(1/sqrt 2), the
 *                              step digifil runs between Rescale and the digitizer (LoadToFil.C:333-343); out of place. */
int dspsr_amd_pscrunch_tfp(dspsr_amd_ctx* ctx, const float* in_tfp_dev, float* out_tfp_dev, uint64_t ndat, uint32_t nchan,
                           uint32_t npol);
typedef struct dspsr_amd_rescale dspsr_amd_rescale;
int dspsr_amd_rescale_create(dspsr_amd_ctx* ctx, uint32_t nchan, uint32_t npol, uint64_t interval_samples, int constant,
                             dspsr_amd_rescale** out);
void dspsr_amd_rescale_destroy(dspsr_amd_rescale* r);
int dspsr_amd_rescale_transform(dspsr_amd_rescale* r, const float* in_tfp_dev, float* out_tfp_dev, uint64_t ndat);
int dspsr_amd_rescale_get(dspsr_amd_rescale* r, float* offset_host, float* scale_host);   /* [npol*nchan]: index ichan*npol+ipol */
/* digifil's whole output stage behind the TFP filterbank (LoadToFil.C:318-362) in one pass over a PPQQ block [ndat][nchan][2]:
 * dsp::Rescale (statistics and intervals exactly as dspsr_amd_rescale_transform, Rescale.C:217-388) -> dsp::PScrunch
 * (PScrunch.C:52,72-90) -> dsp::SigProcDigitizer::pack (SigProcDigitizer.C:112-236; nbit 1/2/4/8/16, input scale 1 behind Rescale),
 * the same float operations in the same order as the three separate calls -- identical bytes -- without writing the rescaled
 * and the summed block.  out_dev: [ndat][nchan * nbit / 8] bytes.
 * in_tfp_dev must be 8-byte aligned (the two polarisations of a channel are read as one float2; a PPQQ sample is 8 bytes, so any
 * sample of an 8-byte aligned block qualifies): a block that is only float aligned is refused with DSPSR_AMD_EINVAL before any launch
 * and the Rescale state stays as it was -- such a block takes the three separate calls, which accept any float address. */
int dspsr_amd_rescale_pscrunch_digitize(dspsr_amd_rescale* r, const float* in_tfp_dev, uint64_t ndat, int nbit, float scale_fac,
                                        int flip_band, int swap_band, void* out_dev);
int dspsr_amd_sigproc_digitize(dspsr_amd_ctx* ctx, const float* in_tfp_dev, uint64_t ndat, uint32_t nchan, uint32_t npol,
                               int nbit, int use_digi_scales, double input_scale, float scale_fac, int flip_band,
                               int swap_band, void* out_dev);
/* The same two operations on FPT-ordered rows [nchan][npol] of ndat floats -- what digifil's convolving branch hands them (the
 * Filterbank keeps the reference's FPT order): Rescale.C:232-262,330-347 (FPT branches; the statistics, intervals and offset /
 * scale arrays are those of the TFP form: one dspsr_amd_rescale object serves either order, index ichan*npol + ipol) and
 * SigProcDigitizer.C:238-290 (FPT branch: the bytes leave in the same TPF order as from TFP input, outidx = idat*nchan*npol +
 * ipol*nchan + ichan; pack_float :346-358 for nbit -32).
 * dspsr_amd_rescale_digitize_fpt: both in one pass over the rows (the rescaled block is not written), identical bytes. */
int dspsr_amd_rescale_transform_fpt(dspsr_amd_rescale* r, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                                    float* out_dev, uint64_t out_chan_stride, uint64_t out_pol_stride, uint64_t ndat);
int dspsr_amd_sigproc_digitize_fpt(dspsr_amd_ctx* ctx, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                                   uint64_t ndat, uint32_t nchan, uint32_t npol, int nbit, int use_digi_scales, double input_scale,
                                   float scale_fac, int flip_band, int swap_band, void* out_dev);
int dspsr_amd_rescale_digitize_fpt(dspsr_amd_rescale* r, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                                   uint64_t ndat, int nbit, float scale_fac, int flip_band, int swap_band, void* out_dev);

/* ---- PSRFITS search-mode output stage: dsp::FITSDigitizer (Kernel/Formats/fits/FITSDigitizer.C), digifits' back half -------------
 * One object per output stream.  nbit 1/2/4/8; nsblk = samples per output block (set_rescale_samples); nblock >= 1 = blocks of the
 * running mean (set_rescale_nblock); constant = keep the first block's spectrum (set_rescale_constant); flip_band = input bandwidth
 * > 0, swap_band = input->get_swap() (ChannelSort :116-145, the map of dspsr_amd_sigproc_digitize_fpt).
 * dspsr_amd_fits_digitizer_pack: rescale_pack() of ONE block of exactly nsblk samples, FPT rows [nchan][npol] of floats (strides in
 *   floats): measure_scale (:178-321) over the block, the spectrum applied to the same block, digi_sigma 8, sub-byte samples most
 *   significant bits first.  out_bytes_dev: nsblk*npol*nchan*nbit/8 bytes, sample idat*nchan*npol + ipol*nchan + ichan;
 *   dat_scl_dev / dat_offs_dev: [npol*nchan] floats of get_scales (:675-699), index ipol*nchan + ichan (output channel).
 *   Three launches on the context's stream, no host synchronisation.
 * Refused with DSPSR_AMD_EINVAL before any launch: any other nbit; nchan not a multiple of 8/nbit (a byte would straddle two
 *   polarisations); nsblk 0 or > 2^30; nblock 0; nchan*npol > 65535 (the grid limit of the FPT digitiser); rows shorter than nsblk or
 *   overlapping; pointers that are null or not float aligned. */
typedef struct dspsr_amd_fits_digitizer dspsr_amd_fits_digitizer;
int dspsr_amd_fits_digitizer_create(dspsr_amd_ctx* ctx, uint32_t nchan, uint32_t npol, int nbit, uint32_t nsblk, uint32_t nblock,
                                    int constant, int flip_band, int swap_band, dspsr_amd_fits_digitizer** out);
void dspsr_amd_fits_digitizer_destroy(dspsr_amd_fits_digitizer* d);
int dspsr_amd_fits_digitizer_pack(dspsr_amd_fits_digitizer* d, const float* in_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                                  void* out_bytes_dev, float* dat_scl_dev, float* dat_offs_dev);

/* ---- host-side preparation (stays on the host in the reference as well) --------------------- */
typedef struct {
  double centre_frequency;   /* MHz */
  double bandwidth;          /* MHz, signed */
  double dispersion_measure;
  uint32_t input_nchan;
  uint32_t nchan;            /* output channels */
  uint32_t ndim;             /* input ndim: 1 Nyquist, 2 Analytic */
  int32_t dual_sideband;     /* -1 unset (Observation.C:80-87) */
  uint32_t dc_centred;
  uint32_t swap;
  uint32_t freq_res;         /* 0 => optimal (optimize_fft.c) else -x value (checked like Response.C:328-344) */
  uint32_t ndat_max;         /* Response::ndat_max, 0 => none */
  uint32_t fractional_delay; /* -K: add the fractional-sample inter-channel delay phase (Dedispersion.C:524-545,
                                set by LoadToFold1.C:605-624); the integer part is dsp::SampleDelay's job */
} dspsr_amd_dedispersion_config;

typedef struct {
  uint32_t impulse_pos, impulse_neg;   /* Dedispersion.C:216-248 */
  uint32_t minimum_ndat;               /* Response.C:259-275 */
  uint32_t ndat;                       /* chosen frequency resolution */
} dspsr_amd_dedispersion_info;

/* Dedispersion::prepare + resolution choice; error if -x is below the minimum (Response::check_ndat) */
int dspsr_amd_dedispersion_prepare(const dspsr_amd_dedispersion_config* cfg, dspsr_amd_dedispersion_info* info,
                                   char* errbuf, size_t errlen);
/* Dedispersion::build + Response::match ordering (Dedispersion.C:261-331,478-556; Response.C:132-181):
 * kernel_host receives nchan*ndat complex floats */
int dspsr_amd_dedispersion_build(const dspsr_amd_dedispersion_config* cfg, uint32_t ndat, float* kernel_host);
/* Dedispersion::SampleDelay::match (DedispersionSampleDelay.C:24-75): delay of each channel in samples relative to the
 * centre frequency, channel frequencies as Observation::get_centre_frequency(ichan) (Observation.C:420-451) */
int dspsr_amd_dedispersion_sample_delays(double centre_frequency, double bandwidth, double dispersion_measure,
                                         uint32_t nchan, double rate_hz, int swap, uint32_t nsub_swap, int dc_centred,
                                         int64_t* delays_host);
uint64_t dspsr_amd_optimal_fft_length(uint64_t nbadperfft, uint64_t nfft_max);           /* optimize_fft.c:63-127 */
/* (int8+0.5)*scale constant of the 8-bit LUT (BitTable.C:165-218) for a given JA98 spacing (ext) */
double dspsr_amd_eight_bit_scale(double ja98_spacing);
/* bin plan of Fold.C:744-787: binplan[ndat] and hits[nbin] += */
int dspsr_amd_fold_binplan(double phi, double phase_per_sample, uint32_t nbin, uint64_t ndat,
                           uint32_t* binplan_host, uint32_t* hits_host);
/* the same plan as its runs (first sample, bin, samples; at most `cap` stored, *nruns = how many there are), found per run
 * instead of per sample -- the values of the recurrence, not an approximation (csrc/host_prep.cpp fold_plan_run); what
 * dspsr_amd_fold_set_bins builds its plan with */
int dspsr_amd_fold_binplan_runs(double phi, double phase_per_sample, uint32_t nbin, uint64_t ndat, uint64_t* run_offset,
                                uint32_t* run_bin, uint64_t* run_hits, uint64_t cap, uint64_t* nruns, uint32_t* hits_host);

/* the two plans of lag folding (CyclicFold.C:293-301 fed by Fold.C:744-787): plan0[ndat], plan1[ndat], hits[nbin] += (may be NULL) */
int dspsr_amd_cyclic_binplan(double phi, double phase_per_sample, uint32_t nbin, uint64_t ndat, uint32_t* plan0_host,
                             uint32_t* plan1_host, uint32_t* hits_host);
/* dsp::CyclicFoldEngine::synch (CyclicFold.C:450-555) on the host, once per sub-integration as in the reference: per (bin, pol,
 * chan), for mover > 1 the window 0.5 (1 + cos(2 pi l / (2 nlag))) sin(x) / x, x = (pi / 3) mover l / (2 nlag - 2), on lags l >= 1
 * (:519-537, float arithmetic), then an unnormalised backward complex-to-real transform of nchan_spec = 2 nlag - 2 points
 * (FTransform bcr1d), every mover-th point kept (:539-546):
 *   lags_host [bin][pol][chan][lag][re, im]  ->  out_host [chan * nchan_spec / mover + schan][pol][bin]
 * nchan_spec must be a power of two (and a multiple of mover): anything else DSPSR_AMD_EINVAL. */
int dspsr_amd_cyclic_lags_to_spectra(const float* lags_host, uint32_t nchan, uint32_t npol, uint32_t nbin, uint32_t nlag,
                                     uint32_t mover, float* out_host);

/* ---- dspsr -R: dsp::RFIFilter (Signal/General/RFIFilter.C) -- host code, no device call ------------------------------------
 * rfi_mask_calculate : RFIFilter::calculate (:105-162) on the integrated passband of the two polarisations, p0[n] and p1[n] (both
 *                      zeroed where zapped, as the reference does); mask[n] receives the 0/1 response.
 *                      keep_zapped = 0 is the reference's loop to the letter: every round sets a channel that does not trigger
 *                      to 1, also one zapped earlier, and the loop ends after a round without a trigger -- the mask is all ones
 *                      whatever the data.  keep_zapped = 1: a channel zapped in any round stays 0.
 *                      total_zapped counts re-zaps as the reference does; rounds = rounds run.
 *                      DSPSR_AMD_ESTATE: a round re-zapped channels and zapped no new one -- with a cutoff below zero the
 *                      reference's loop repeats that round for ever.
 *                      fft::median_smooth is PSRCHIVE's, restated: odd window, computed from the unmodified data, truncated at the
 *                      edges, element len/2 of the sorted window.
 * _log               : the same, and the cutoff of every round (at most cutoff_cap stored): "round k cutoff = ..." of :142
 * rfi_mask_expand    : RFIFilter::match (const Response*) (:165-206): expand = required / n in integers, elements past n*expand
 *                      stay 1; required < n leaves all ones (the shrink loop's bound is `expand`, which is 0 there).
 *                      phasors: `required` complex floats, imaginary part 0
 * response_multiply  : Response::operator *= (Response.C:73-104, :429-441): kernel[i] = phasors[i] * kernel[i]; a phasor (1, 0)
 *                      leaves a finite kernel unchanged bit for bit, except for the sign of a zero */
int dspsr_amd_rfi_mask_calculate(float* p0, float* p1, uint32_t n, uint32_t median_window, int keep_zapped, float* mask,
                                 uint32_t* total_zapped, uint32_t* rounds);
int dspsr_amd_rfi_mask_calculate_log(float* p0, float* p1, uint32_t n, uint32_t median_window, int keep_zapped, float* mask,
                                     uint32_t* total_zapped, uint32_t* rounds, float* cutoffs, uint32_t cutoff_cap);
int dspsr_amd_rfi_mask_expand(const float* mask, uint32_t n, uint64_t required, float* phasors);
int dspsr_amd_response_multiply(float* kernel, const float* phasors, uint64_t ncomplex);
#ifdef __cplusplus
}
#endif
#endif /* DSPSR_AMD_H */
