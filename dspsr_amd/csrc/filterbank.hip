// Convolving filterbank (dsp::Filterbank -F N:D), host side: geometry, kernel choice and the launch sequence per call.
// Kernels: fb_fwd_cols.hip, fb_fwd_rows.hip, fb_inv_chan*.hip, fb_two_pass.hip, fb_four_pass.hip; shared: fb_common.h
#include "fb_common.h"
#include "fb_rows.h"
#include <initializer_list>

namespace dspsr_amd {

constexpr int LOG_POINTS_DEFAULT = 14;  // points per workgroup (32 per thread, 512 threads)

static inline int ilog2(uint64_t v) { int l = 0; while ((1ull << l) < v) l++; return l; }
static inline bool ispow2(uint64_t v) { return v && !(v & (v - 1)); }

// One pass as the host launches it (fb_launch): the kernel chosen for this geometry (nullptr: there is none), its workgroup, its
// dynamic LDS and how many of its workgroups a compute unit holds -- the persistent grid is at most ncu * wg_per_cu
template <class K> struct FbPass { K kern; uint32_t threads; size_t lds; uint32_t wg_per_cu; };

struct dspsr_amd_filterbank_impl {
  dspsr_amd_ctx* ctx;
  dspsr_amd_filterbank_config cfg;
  FbGeom g;
  uint64_t N, L;
  uint32_t nseq, max_parts, ncu;
  uint64_t part_elems = 0;    // scratch elements per part
  cf* A = nullptr;
  cf* X = nullptr;
  cf* kernel = nullptr;
  cf* tw_lo = nullptr;
  cf* tw_lo_m = nullptr;
  uint16_t* Rt = nullptr;   // pre-transposed 8-bit pairs of the parts of one launch group
  PlanSlot* plan_wait = nullptr;             // fold plan on its way to the device: the first kernel that reads it waits (fold_plan_wait)
  float* det = nullptr;     // detected block of perform_fold when the fused kernel would not fill the chip
  size_t det_floats = 0;
  bool kernel_set = false;
  float4* rmatrix = nullptr;  // matrix response (set_response_matrix): nchan_subband * freq_res bins of two float4, (f11, f21) (f22, f12)
  // the passes of this geometry: shapes from fb_tile, kernels chosen and given their dynamic-LDS limit once, at create time
  FbPass<k1_t> p1_w1 = {}, p1_w4 = {};       // pass 1: one word per sample pair / generic loads
  FbPass<k1_t> p1d_w1 = {}, p1d_w4 = {};     // ... on pairs of tiles (64-byte A runs otherwise), see k_fwd_cols_dual
  FbPass<k2_t> p2 = {};
  FbPass<k3_t> p3 = {}, p3f = {}, p3s = {};  // inverse pass: plain, fused fold (the plan in LDS behind the tile), search mode
  FbPass<k3_t> p3m = {};                     // ... with the matrix response (fb_pick3m; set by the first set_response_matrix)
  FbPass<k3_t> p3q = {};                     // ... fused fold of the square-law states (Intensity, PPQQ): p3f's LDS and plan
  FbPass<k3_t> p3c = {};                     // ... search mode on the four Coherence products (fb_pick3c): p3s's shape
  FbPass<k3a_t> p3a = {};                    // four-pass geometry: the first inverse pass
  FbPass<k3b_t> p3b = {}, p3bf = {};         // ... the second one, plain / leaving fold segment sums (FB_OUT_SEGSUM)
  float* fpart = nullptr;    // segmented fused fold: partial profiles of the part runs 1 .. nseg-1 of a launch
  size_t fpart_floats = 0;
  uint32_t plan_cap = 0;     // fused fold: plan entries per LDS buffer behind the twiddle tables
  // two-pass path of short responses (complex dual-pol 8-bit input, nchan_subband * freq_res^2 == 2^27): see fb_two_pass.hip
  uint8_t* dsub = nullptr;    // nsub > 1: the launch group's samples de-interleaved into nsub blocks (k_sub_split)
  size_t dsub_bytes = 0;
  bool two_pass = false;
  bool presplit = false;      // three-pass path on the pre-split spectrum (fb_takes_presplit): p1_*, p2, p3* are the kernels of that form
  FbPass<k1c_t> p1c = {};     // two-pass path, Fa = 2^14: pass 1 on whole columns
  FbGeom g1t;                 // ... Fa < 2^14: through k_raw_transpose + k_fwd_cols, their geometry (M = Fa, Rr = Fb, T2 = freq_res)
  FbPass<k1_t> p1t = {};
  FbPass<k3_t> p2r = {}, p2rf = {}, p2rs = {};   // ... rows + inverse pass: plain, fused fold, search mode
  FbPass<k3_t> p2rc = {};                        // ... search mode on the four Coherence products
  uint32_t plan_cap2 = 0;
  float* msum = nullptr;     // four-pass fused fold: segment sums [chan][part][tile][t2][2] float4 of one input channel's sub-band and one block
  size_t msum_floats = 0;
  // freq_res = 3 * 2^k / 5 * 2^k (msub = 3, 5; see k_time_combine): g and everything above describe the INNER filterbank of
  // nchan_subband * msub pseudo-channels with freq_res / msub bins and the whole transform kept; cfg and these the caller's
  uint32_t msub = 0, out_C = 0, out_M = 0, out_nfilt_pos = 0, out_nkeep = 0;
  dspsr_amd_filterbank* batch = nullptr;   // dsp::Convolution on many channels (nchan_subband = 1, complex float rows): the inverse passes of a
                             // filterbank of `batch->cfg.nchan_subband` channels per group, see fb_run_batched
  int conv1_logM = -1;       // >= 0: dsp::Convolution shapes with n_fft <= 8192 on complex float rows run in ONE tile pass (fb_conv1.hip)
  int conv3_logM = -1;       // >= 0: ... with 2^14 <= n_fft <= 2^21 in THREE tile passes (fb_conv3.hip), launch groups of conv3_ch channels x
  uint32_t conv3_ch = 0, conv3_parts = 0;    //   conv3_parts parts through the scratch blocks S1 / S2
  cf* S1 = nullptr;
  cf* S2 = nullptr;
  uint64_t conv3_bytes = 0;                  //   bytes of each (allocated on first use; a failed allocation turns the path off)
  cf* kernel_nat = nullptr;  // ... its response in natural order when `kernel` is stored in the blocked order of the four-pass kernels
  int plain_logC = -1;       // >= 0: freq_res = 1, the non-convolving filterbank (fb_plain.hip): no scratch, one launch per call
  cf* Xp = nullptr;          // the combined spectrum in pseudo-channel order (k_sub_combine writes it there)
  cf* Y = nullptr;           // the pseudo-channels' time series of one launch group [pseudo-channel][pol][part][freq_res / msub]
  size_t Xp_elems = 0, Y_elems = 0;
};

}  // namespace dspsr_amd

using namespace dspsr_amd;

struct dspsr_amd_filterbank : dspsr_amd_filterbank_impl {};

static int fb_fail(dspsr_amd_ctx* ctx, int code, const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  ctx_set_error_v(ctx, fmt, ap);
  va_end(ap);
  return code;
}

// dynamic-LDS limits of a geometry's passes, set in order up to the first failure; absent kernels (nullptr) are skipped
template <class... K> static hipError_t allow_lds(const FbPass<K>&... passes)
{
  hipError_t e = hipSuccess;
  ((e = passes.kern && e == hipSuccess ? dspsr_amd_allow_lds((const void*)passes.kern, passes.lds) : e), ...);
  return e;
}

static uint32_t odd_part(uint32_t v) { while (v && !(v & 1)) v >>= 1; return v; }
// (any odd factor up to ODD_MAX: 3, 5, 7, 9, 15 have radix kernels of their own, the others -- 11, 13, 21, 25, ... -- the
//  run-time-radix forms k_sub_combine_any / k_time_combine<0>)
static bool radix_ok(uint32_t r) { return (r & 1u) && r >= 3 && r <= ODD_MAX; }

// the non-convolving filterbank (Filterbank.C:614-623, `dspsr -F N`): nchan_subband-point forward transforms, bin k of a part
// is the part's one output sample of channel k
static int fb_create_plain(dspsr_amd_ctx* ctx, const dspsr_amd_filterbank_config* cfg, dspsr_amd_filterbank** out)
{
  if (cfg->nfilt_pos || cfg->nfilt_neg)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: nfilt_pos+nfilt_neg=%u >= freq_res=1",
                   cfg->nfilt_pos + cfg->nfilt_neg);
  if (!ispow2(cfg->nchan_subband) || cfg->nchan_subband < 2 || cfg->nchan_subband > (1u << MAX_LOGF))
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: freq_res=1 (non-convolving filterbank) needs nchan_subband=%u "
                   "to be a power of two in [2, %u]", cfg->nchan_subband, 1u << MAX_LOGF);
  if (cfg->input_nchan == 0) return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: input_nchan=0");
  const int logC = ilog2(cfg->nchan_subband);
  const int rc = fb_plain_check(ctx, logC, cfg->real_input != 0, cfg->npol, nullptr);
  if (rc != DSPSR_AMD_OK)
    return fb_fail(ctx, rc, "dspsr_amd_filterbank_create: no kernel for the %u-channel non-convolving filterbank", cfg->nchan_subband);
  dspsr_amd_filterbank* fb = new dspsr_amd_filterbank;
  fb->ctx = ctx;
  fb->cfg = *cfg;
  fb->plain_logC = logC;
  fb->N = cfg->nchan_subband;
  fb->L = cfg->real_input ? 2 * fb->N : fb->N;
  fb->nseq = cfg->real_input ? 1 : cfg->npol;
  fb->ncu = ctx->ncu;
  fb->max_parts = cfg->max_parts ? cfg->max_parts : 1;
  FbGeom& g = fb->g;
  g = FbGeom();
  g.real_input = cfg->real_input ? 1 : 0;
  g.npol = cfg->npol;
  g.C = cfg->nchan_subband;
  g.nsub = 1;
  g.nfilt_pos = 0;
  g.nkeep = 1;
  g.xstride = fb->L;
  *out = fb;
  return DSPSR_AMD_OK;
}

// odd factors of freq_res and nchan_subband (0 / 1: none), and the sizes the geometry is built from
struct FbFactors { uint32_t msub, nsub, nchan_sb, fres, nfpos, nfneg; };

// freq_res: a power of two, or 3 or 5 times one with a power-of-two nchan_subband (dspsr -x 12288).  The transforms inside a
// tile stay powers of two: bins m = R m' + r of a channel are R pseudo-channels of freq_res / R bins (the inner filterbank of
// nchan_subband * R channels below, whole transforms kept), whose time series k_time_combine adds with the twiddles
// exp(+2 pi i r n / freq_res) -- the decimation-in-frequency form of the freq_res-point backward transform.
// (odd factors up to ODD_MAX = 127 of either length; both lengths at once as long as the product of the two factors stays within it)
static int fb_check_factors(dspsr_amd_ctx* ctx, const dspsr_amd_filterbank_config* cfg, FbFactors* f)
{
  uint32_t msub = 0;
  if (!ispow2(cfg->freq_res)) {
    msub = odd_part(cfg->freq_res);
    if (!radix_ok(msub) || cfg->nchan_subband == 0 || !(ispow2(cfg->nchan_subband) || radix_ok(odd_part(cfg->nchan_subband) * msub)) ||
        cfg->freq_res / msub < 2 || cfg->force_four_pass == 1)
      return fb_fail(ctx, DSPSR_AMD_EINVAL,
                     "dspsr_amd_filterbank_create: freq_res=%u must be 2^k >= 2, or 2^k (k >= 1) times an odd number <= 127 (times the odd "
                     "factor of nchan_subband=%u: again <= 127)",
                     cfg->freq_res, cfg->nchan_subband);
  } else if (cfg->freq_res < 2)
    return fb_fail(ctx, DSPSR_AMD_EINVAL,
                   "dsp::Filterbank::make_preparations Response.ndat = 0 (freq_res=%u)", cfg->freq_res);
  if (cfg->nfilt_pos + cfg->nfilt_neg >= cfg->freq_res)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: nfilt_pos+nfilt_neg=%u >= freq_res=%u",
                   cfg->nfilt_pos + cfg->nfilt_neg, cfg->freq_res);
  // (the geometry below is built from these: the caller's values, or the inner filterbank's)
  const uint32_t nchan_sb = msub ? cfg->nchan_subband * msub : cfg->nchan_subband, fres = msub ? cfg->freq_res / msub : cfg->freq_res,
                 nfpos = msub ? 0u : cfg->nfilt_pos, nfneg = msub ? 0u : cfg->nfilt_neg;
  // nchan_subband: a power of two, or 3 or 5 times one (the forward transform then runs as 3 / 5 interleaved sub-sequences,
  // k_sub_split / k_sub_combine).
  uint32_t nsub = 1;
  if (!ispow2(nchan_sb)) {
    nsub = nchan_sb ? odd_part(nchan_sb) : 0;
    if (!radix_ok(nsub))
      return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: nchan_subband=%u must be 2^k or 2^k times an odd number <= 127",
                     cfg->nchan_subband);
    if (cfg->force_four_pass == 1)
      return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: nchan_subband=%u (not a power of two) has no four-pass form",
                     cfg->nchan_subband);
  }
  if (cfg->input_nchan == 0) return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: input_nchan=0");
  *f = {msub, nsub, nchan_sb, fres, nfpos, nfneg};
  return DSPSR_AMD_OK;
}

// the transform's sizes and the geometry fields every path shares
static void fb_init_geom(dspsr_amd_filterbank* fb, const FbFactors& f)
{
  const dspsr_amd_filterbank_config* cfg = &fb->cfg;
  FbGeom& g = fb->g;
  // (C, Rr describe the power-of-two geometry passes 0-2 run on: one of nsub sub-sequences; fb->N, fb->L and g.C are the whole
  //  transform's)
  const uint64_t M = f.fres;
  fb->msub = f.msub;
  fb->out_C = cfg->nchan_subband; fb->out_M = cfg->freq_res; fb->out_nfilt_pos = cfg->nfilt_pos;
  fb->out_nkeep = cfg->freq_res - cfg->nfilt_pos - cfg->nfilt_neg;
  fb->N = (uint64_t)f.nchan_sb * M;
  fb->L = cfg->real_input ? 2 * fb->N : fb->N;
  fb->nseq = cfg->real_input ? 1 : cfg->npol;
  g.logM = g.logMf = ilog2(M);
  g.logR = ilog2(fb->L / f.nsub / M);
  g.four_pass = 0; g.xblocked = 0; g.xblock = g.kblock = 0; g.xstride = fb->L;
  g.logMa = g.logMb = g.logTm = g.logTt = 0; g.logFb2 = g.logFa2 = 0;
  g.tw_lo = g.tw_lo_m = nullptr;
  g.real_input = cfg->real_input ? 1 : 0; g.npol = cfg->npol;
  g.C = f.nchan_sb; g.nsub = f.nsub; g.nfilt_pos = f.nfpos; g.nkeep = f.fres - f.nfpos - f.nfneg;
}

// Tiles: every workgroup holds min(2^14, available) points = 32 per thread.  Three passes when freq_res and the spectrum rows
// each fit one workgroup tile, four otherwise; sets the passes' tiles, threads and LDS.
static int fb_tile(dspsr_amd_filterbank* fb)
{
  FbGeom& g = fb->g;
  const uint64_t M = 1ull << g.logMf, C = g.C / g.nsub;
  const int logMf = g.logMf, logL = g.logM + g.logR, logC = ilog2(C);
  constexpr int LOG_POINTS = LOG_POINTS_DEFAULT;
  auto imin = [](int a, int b) { return a < b ? a : b; };
  const int logPol = 1;   // the inverse passes always carry (pol0, pol1) column pairs
  // three passes (freq_res and the spectrum rows each fit one workgroup tile) when possible ...
  uint64_t p1 = 0, p2 = 0, p3 = 0, p4 = 0;
  bool three_ok = g.logM <= MAX_LOGF && g.logR <= MAX_LOGF;
  if (three_ok) {
    g.logT1 = imin(g.logR, LOG_POINTS - g.logM);
    g.logT2 = imin(g.logM, LOG_POINTS - g.logR);
    int t3 = LOG_POINTS - g.logM - logPol;
    if (t3 < 0) t3 = 0;
    g.logX3 = imin(logC, t3);                    // X layout: keeps the pass-2 store runs at T2*X3 elements
    g.logT3 = g.logX3;                           // pass-3 tile = one layout block
    p1 = M << g.logT1; p2 = (1ull << g.logR) << g.logT2; p3 = (M << g.logT3) << logPol;
    three_ok = !(p1 < 32 || p2 < 32 || p3 < 32 || p3 > (1u << LOG_POINTS) || g.logT1 < 1 || g.logT2 < 1);
  }
  // ... otherwise four: L = Fa*Fb forward (whole spectrum, blocked by pass-2 tile), freq_res = Ma*Mb inverse in two passes.
  // This also covers nchan_subband = 1 (dsp::Convolution) and freq_res up to 2^26.
  if (g.nsub > 1 && !three_ok)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: nchan_subband=%u (not a power of two) needs freq_res <= 8192 "
                   "and a sub-geometry of at least 32 points per pass", fb->cfg.nchan_subband);
  if (fb->cfg.force_four_pass == 1 || !three_ok) {
    int la = (logL + 1) / 2;
    if (la > MAX_LOGF) la = MAX_LOGF;
    const int lb = logL - la;
    // spectrum layout between pass 2 and the inverse: blocked (every pass-2 tile one contiguous block) when the natural
    // order would leave pass 2 with runs of fewer than 16 elements (128 bytes); measured per geometry, blocked is then
    // 15-40 % faster over the whole launch group, natural 3 % faster otherwise (profiles/r02x_inverse_split.txt)
    const int logT2f = imin(la, LOG_POINTS - (logL - la));
    const bool blocked = logT2f < 4;
    // freq_res = Ma*Mb: the split that measured fastest (same file).  The second inverse pass likes Mb = 256 (two
    // radix-16 stages, 32 adjacent output samples per run), the first one Ma <= 2^11 (>= 4 columns per tile).
    static const signed char lma_best[27] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 7, 8, 9, 10, -1, 10, 11, 11, 11, 12, 12, 13};
    int lma = (logMf + 1) / 2;
    if (logMf >= 14 && logMf <= 26) lma = lma_best[logMf] > 0 ? lma_best[logMf] : (blocked ? 11 : 9);
    if (lma > MAX_LOGF) lma = MAX_LOGF;
    const int lmb = logMf - lma;
    g.logM = la; g.logR = lb; g.logT3 = g.logX3 = 0;
    g.logT1 = imin(lb, LOG_POINTS - la);
    g.logT2 = imin(la, LOG_POINTS - lb);
    g.logMa = lma; g.logMb = lmb;
    g.logTm = imin(lmb, LOG_POINTS - logPol - lma);
    g.logTt = imin(lma, LOG_POINTS - logPol - lmb);
    p1 = (1ull << la) << g.logT1; p2 = (1ull << lb) << g.logT2;
    p3 = ((1ull << lma) << g.logTm) << logPol; p4 = ((1ull << lmb) << g.logTt) << logPol;
    const bool ok = lb >= 1 && lb <= MAX_LOGF && lmb >= 1 && lmb <= MAX_LOGF && g.logT1 >= 1 && g.logT2 >= 1 &&
                    g.logTm >= 0 && g.logTt >= 0 && p1 >= 32 && p2 >= 32 && p3 >= 32 && p4 >= 32;
    if (!ok)
      return fb_fail(fb->ctx, DSPSR_AMD_EINVAL,
                     "dspsr_amd_filterbank_create: nchan_subband=%llu freq_res=%llu cannot be tiled "
                     "(forward 2^%d x 2^%d, inverse 2^%d x 2^%d; every pass needs 32..16384 points per workgroup "
                     "and factors <= 2^%d)", (unsigned long long)C, (unsigned long long)M, la, lb, lma, lmb, MAX_LOGF);
    g.four_pass = 1;
    // (k_inv_a's address arithmetic assumes that a thread's 16 elements differ in bits of k above the low T2 ones)
    g.xblocked = (blocked && lmb >= g.logT2 && (p3 / PTS) >= (1u << g.logT2)) ? 1 : 0;
    if (g.xblocked) {
      g.xblock = 1u << (lb + g.logT2);           // (padding between the blocks measured irrelevant: profiles/r04_experiments.txt item 12)
      g.xstride = (uint64_t)g.xblock << (la - g.logT2);
      g.kblock = (uint32_t)((fb->N >> la) << g.logT2);
    }
  }
  // a tile of `points` points transformed over 2^logn: PTS points per thread; workgroups per compute unit: two of a small tile
  auto shape = [](auto& pass, uint64_t points, int logn, bool two_fit) {
    pass = {nullptr, (uint32_t)(points / PTS), lds_total_words_host((uint32_t)points, logn) * sizeof(cf), 1};
    if (two_fit && 2 * pass.lds + 1024 <= 160 * 1024) pass.wg_per_cu = 2;
  };
  shape(fb->p1_w1, p1, g.logM, p1 / PTS <= 256);
  fb->p1_w4 = fb->p1d_w1 = fb->p1d_w4 = fb->p1_w1;
  shape(fb->p2, p2, g.logR, false);
  if (g.four_pass) {
    shape(fb->p3a, p3, g.logMa, false);
    shape(fb->p3b, p4, g.logMb, false);
    fb->p3bf = fb->p3b;
  } else {
    shape(fb->p3, p3, g.logM, true);
    fb->p3f = fb->p3q = fb->p3s = fb->p3c = fb->p3m = fb->p3;
  }
  return DSPSR_AMD_OK;
}

// Pre-split spectrum (fb_row_map.h): pass 1 leaves the rows of A in mirror-paired blocks, pass 2 forms the Hermitian
// split and stores the two polarisations, the inverse pass loads them ready.  Taken for real dual-polarisation input on the
// three-pass path of a power-of-two geometry (nsub == 1, no odd factor of freq_res either: those spectra pass through
// k_sub_combine in the X layout), unless pass 1 runs on pairs of tiles (k_fwd_cols_dual stages its image itself) or the caller
// asked for the split in the inverse pass.  The tile arithmetic needs no more: a pass-2 tile holds T2 >= 2 rows, i.e. T2 / 2 >= 1
// mirror pairs, and its T2 * Rr / 2 outputs of 16 bytes are the 16 per thread the copy-out writes.
static bool fb_takes_presplit(const dspsr_amd_filterbank* fb, bool dual)
{
  const FbGeom& g = fb->g;
  return fb->cfg.split_in_inverse == 0 && g.real_input && g.npol == 2 && g.nsub == 1 && !fb->msub && !g.four_pass && !dual &&
         g.logT2 >= 1 && g.logT2 <= g.logM;
}

// kernels of this geometry and their dynamic-LDS limits (once; perform only launches)
static int fb_pick_kernels(dspsr_amd_filterbank* fb)
{
  const FbGeom& g = fb->g;
  const bool full1 = g.logT1 == full_logt(g.logM), full2 = g.logT2 == full_logt(g.logR),
             full3 = !g.four_pass && g.logT3 + 1 == full_logt(g.logM);
  // two-column tiles of 2^13 rows whose A runs would be half cache lines: transformed in pairs (k_fwd_cols_dual)
  const bool dual = full1 && g.logM == 13 && g.logT1 == 1 && g.logT1 + g.logT2 < 4 && g.logR >= 2;
  const bool ps = fb->presplit = fb_takes_presplit(fb, dual);
  fb->p1_w1.kern = ps ? fb_pick1_rm(g.logM, 1, full1) : fb_pick1(g.logM, 1, full1);
  fb->p1_w4.kern = ps ? fb_pick1_rm(g.logM, 4, full1) : fb_pick1(g.logM, 4, full1);
  fb->p1d_w1.kern = dual ? fb_pick1_dual(1) : nullptr;
  fb->p1d_w4.kern = dual ? fb_pick1_dual(4) : nullptr;
  fb->p2.kern = fb_pick2(g.logR, full2, ps);
  if (g.four_pass) {
    fb->p3a.kern = fb_pick3a(g.logMa, g.xblocked != 0, g.real_input != 0, g.logTm == 13 - g.logMa && g.logMa <= 12 && fb->p3a.threads == 512);
    const bool full4 = g.logTt == 13 - g.logMb && g.logMb <= 12 && fb->p3b.threads == 512;
    fb->p3b.kern = fb_pick3b(g.logMb, false, full4);
    fb->p3bf.kern = fb_pick3b(g.logMb, true, full4);
  } else {
    fb->p3.kern = fb_pick3(g.logM, full3, ps);
    fb->p3f.kern = fb_pick3f(g.logM, full3, ps);
    fb->p3s.kern = fb_pick3s(g.logM, full3, ps);
    fb->p3c.kern = fb_pick3c(g.logM, full3, ps);
    // fused fold: the LDS left over behind the twiddle tables holds the part's fold plan (two buffers)
    const FbPlanLds pl = fb_plan_lds(fb->p3.lds, fb->p3.threads);   // one plan entry per thread of the workgroup (<= 512)
    fb->plan_cap = pl.cap;
    fb->p3f.lds = pl.lds;
    fb->p3q.kern = fb_pick3q(g.logM, full3, ps);
    fb->p3q.lds = pl.lds;
  }
  if (!((fb->p1_w1.kern || fb->p1_w4.kern) && fb->p2.kern && (g.four_pass ? (fb->p3a.kern && fb->p3b.kern) : (fb->p3.kern != nullptr))))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: no kernel for this geometry");
  // (the three passes of the pre-split form only work together: X' is not the X layout; it takes the L elements per part X has)
  if (ps && !(fb->p1_w1.kern && fb->p1_w4.kern && fb->p3f.kern && fb->p3s.kern && fb->nseq == 1 && g.xstride == fb->L))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: no kernels for the pre-split spectrum of this geometry");
  const hipError_t e = allow_lds(fb->p1_w1, fb->p1_w4, fb->p1d_w1, fb->p1d_w4, fb->p2, fb->p3, fb->p3f, fb->p3q, fb->p3s, fb->p3c, fb->p3a, fb->p3b, fb->p3bf);
  if (e != hipSuccess)
    return fb_fail(fb->ctx, DSPSR_AMD_EHIP, "dspsr_amd_filterbank_create: hipFuncSetAttribute: %s", hipGetErrorString(e));
  return DSPSR_AMD_OK;
}

// Two-pass path: forward and inverse levels together fit two workgroup tiles (fb_two_pass.hip).  Complex dual-pol input,
// 512 <= freq_res <= 4096, Fb = 2^13 / freq_res channels per inverse tile, Fa = L / Fb with freq_res <= Fa <= 2^14, i.e.
// Fb <= nchan_subband <= 2^27 / freq_res^2 (the 50 MHz sub-band geometry -F 512:D -x 512 is the upper end).  Taken per call
// when the input is the generic 8-bit block (fb_takes_two_pass); the three-pass kernels above serve every other input form.
// force_four_pass == 2 switches it off (comparison runs and tests).
static void fb_setup_two_pass(dspsr_amd_filterbank* fb)
{
  const dspsr_amd_filterbank_config* cfg = &fb->cfg;
  FbGeom& g = fb->g;
  const int logMf = g.logMf, logL = ilog2(fb->L), lfb = 13 - logMf, lfa = logL - lfb;
  if (!(g.nsub == 1 && !g.four_pass && !cfg->real_input && cfg->npol == 2 && cfg->force_four_pass != 2 && logMf >= 9 && logMf <= 12 &&
        lfa >= logMf && lfa <= 14 && fb->ctx->ncu > 0))
    return;
  hipError_t e = hipSuccess;
  bool have1 = false;
  if (lfa == 14) {
    fb->p1c = {fb_pick_col1(), 512, lds_total_words_host(1u << 14, 12) * sizeof(cf), 1};
    have1 = fb->p1c.kern != nullptr;
    if (have1) e = allow_lds(fb->p1c);
  } else {
    // pass 1 = the ordinary column pass on a geometry of its own: T1 adjacent columns nb per tile, A blocked by T2 = freq_res
    FbGeom& q = fb->g1t;
    q = g;
    q.logM = lfa; q.logR = lfb;
    q.logT1 = lfb < LOG_POINTS_DEFAULT - lfa ? lfb : LOG_POINTS_DEFAULT - lfa;
    q.logT2 = logMf;
    const uint64_t p1t = (1ull << lfa) << q.logT1;
    fb->p1t = {fb_pick1(lfa, 1, q.logT1 == full_logt(lfa)), (uint32_t)(p1t / PTS), lds_total_words_host((uint32_t)p1t, lfa) * sizeof(cf), 1};
    have1 = fb->p1t.kern != nullptr && q.logT1 >= 1 && p1t >= 32;
    if (have1) e = allow_lds(fb->p1t);
  }
  // rows + inverse pass: a full tile, 512 threads, one workgroup per compute unit; the fused fold's plan behind it
  const size_t lds2r = lds_total_words_host(1u << 14, logMf) * sizeof(cf);
  const FbPlanLds pl = fb_plan_lds(lds2r, 512);
  fb->p2r = {fb_pick_rinv(logMf, 0), 512, lds2r, 1};
  fb->p2rf = {fb_pick_rinv(logMf, 1), 512, pl.lds, 1};
  fb->p2rs = {fb_pick_rinv(logMf, 2), 512, lds2r, 1};
  fb->p2rc = {fb_pick_rinv(logMf, 4), 512, lds2r, 1};
  if (!(have1 && fb->p2r.kern && fb->p2rf.kern && fb->p2rs.kern && fb->p2rc.kern)) return;
  g.logFb2 = lfb;
  g.logFa2 = lfa;
  fb->g1t.logFb2 = lfb; fb->g1t.logFa2 = lfa;
  fb->plan_cap2 = pl.cap;
  if (e == hipSuccess) e = allow_lds(fb->p2r, fb->p2rf, fb->p2rs, fb->p2rc);
  fb->two_pass = e == hipSuccess;
}

// fine twiddle table exp(-2 pi i j / n), j < 2^sh, built in double, into a device buffer of its own (*dev: freed with the object)
static bool fb_twiddle_table(cf** dev, int sh, double n)
{
  std::vector<cf> lo(1u << sh);
  for (uint32_t j = 0; j < (1u << sh); j++) {
    const double a = -2.0 * M_PI * (double)j / n;
    lo[j] = make_float2((float)cos(a), (float)sin(a));
  }
  return hipMalloc((void**)dev, lo.size() * sizeof(cf)) == hipSuccess &&
         hipMemcpy(*dev, lo.data(), lo.size() * sizeof(cf), hipMemcpyHostToDevice) == hipSuccess;
}

// the scratch blocks A and X of max_parts parts, and the fine twiddle tables
static int fb_alloc_scratch(dspsr_amd_filterbank* fb)
{
  FbGeom& g = fb->g;
  fb->max_parts = fb->cfg.max_parts ? fb->cfg.max_parts : 1;
  // per part: nseq sequences of L points; the two-pass inverse re-uses A for 2 polarisations x N bins
  fb->part_elems = fb->nseq * g.xstride;       // (A needs nseq*L; X the same or, blocked and padded, a little more)
  if (g.four_pass && fb->part_elems < 2 * fb->N) fb->part_elems = 2 * fb->N;
  const size_t scratch = (size_t)fb->max_parts * fb->part_elems * sizeof(cf);
  if (hipMalloc((void**)&fb->A, scratch) != hipSuccess || hipMalloc((void**)&fb->X, scratch) != hipSuccess)
    return fb_fail(fb->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_create: hipMalloc of 2 x %zu scratch bytes failed", scratch);
  // the two-pass inverse's table, then pass 1's
  if ((g.four_pass && g.logMf > LOG_TWN && !fb_twiddle_table(&fb->tw_lo_m, g.logMf - LOG_TWN, (double)(1ull << g.logMf))) ||
      (g.logM + g.logR > LOG_TWN && !fb_twiddle_table(&fb->tw_lo, g.logM + g.logR - LOG_TWN, (double)fb->L)))
    return fb_fail(fb->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_create: twiddle table allocation failed");
  g.tw_lo_m = fb->tw_lo_m;
  g.tw_lo = fb->tw_lo;
  return DSPSR_AMD_OK;
}

// dsp::Convolution shapes (nchan_subband = 1, complex dual-pol): the one-pass, three-pass and grouped paths
static void fb_setup_conv(dspsr_amd_filterbank* fb)
{
  const dspsr_amd_filterbank_config* cfg = &fb->cfg;
  const FbGeom& g = fb->g;
  const bool conv = cfg->nchan_subband == 1 && !cfg->real_input && cfg->npol == 2 && !fb->msub && g.nsub == 1;
  // dsp::Convolution with a short response (n_fft <= 8192) on complex float rows: the whole transform of a (channel, part) sequence,
  // both polarisations, fits one workgroup tile -- forward transform, response, backward transform, keep window and Detection in ONE
  // pass over the rows (fb_conv1.hip) instead of four.  force_four_pass != 0 keeps the four-pass kernels (tests, comparison runs).
  if (conv && cfg->force_four_pass == 0 && g.logMf >= 6 && g.logMf <= 13 && fb_conv1_check(g.logMf, nullptr) == DSPSR_AMD_OK)
    fb->conv1_logM = g.logMf;
  // The same with a response of 2^14 ... 2^21 points: three tile passes instead of four -- the forward transform's second pass and the
  // inverse transform's first one run along the same rows and are one pass (fb_conv3.hip).  Launch groups of channels x parts that fill
  // about 2 GB per scratch buffer.
  if (fb->conv1_logM < 0 && conv && cfg->force_four_pass == 0 &&
      g.logMf >= CONV3_MIN_LOGM && g.logMf <= CONV3_MAX_LOGM && fb_conv3_check(g.logMf) == DSPSR_AMD_OK) {
    const uint64_t seq_bytes = (2ull << g.logMf) * sizeof(cf);           // one (channel, part), both polarisations
    uint64_t max_seq = (2ull << 30) / seq_bytes;
    uint64_t np = fb->max_parts < max_seq ? fb->max_parts : max_seq;
    if (np < 1) np = 1;
    uint64_t ch = max_seq / np;
    if (ch < 1) ch = 1;
    if (ch > cfg->input_nchan) ch = cfg->input_nchan;
    // (the two scratch buffers are allocated by the first call that takes this path: an object fed 8-bit blocks never does)
    fb->conv3_logM = g.logMf;
    fb->conv3_ch = (uint32_t)ch;
    fb->conv3_parts = (uint32_t)np;
    fb->conv3_bytes = np * ch * seq_bytes;
  }
  // dsp::Convolution behind a filterbank (nchan_subband = 1 on many input channels, `dspsr -F N`): one launch group per input channel
  // holds parts x 2 x freq_res points -- a tile or two per compute unit and four launches per channel.  The channels of a GROUP run
  // as one launch group instead (fb_run_batched): forward passes on the group's (part, pol, channel) sequences with this object's
  // per-channel geometry, inverse passes of a `group`-channel filterbank object (natural spectrum order) on the spectra laid side
  // by side.  Complex float32 rows read in place by pass 1; other inputs keep the loop over the channels.
  if (fb->conv1_logM < 0 && fb->conv3_logM < 0 && conv && cfg->input_nchan >= 4 && cfg->force_four_pass != 2 &&
      g.four_pass && !g.xblocked && !(g.logR >= 6 && g.logT1 <= 4) && fb->p1_w4.kern) {
    uint32_t ch = 1;
    while (ch < 64 && cfg->input_nchan % (2 * ch) == 0) ch *= 2;
    // (scratch of the group object: max_parts x 2 x ch x freq_res elements per buffer; keep it near 2 GB)
    while (ch > 2 && (uint64_t)fb->max_parts * 2 * ch * fb->N * sizeof(cf) > (2ull << 30)) ch /= 2;
    // (the group object must keep its spectrum in natural order: ch * freq_res <= 2^21, see `blocked` in fb_tile)
    while (ch > 1 && ilog2(ch) + g.logMf > 21) ch /= 2;
    if (ch >= 2) {
      dspsr_amd_filterbank_config c2 = *cfg;
      c2.nchan_subband = ch;
      c2.input_nchan = cfg->input_nchan / ch;
      c2.force_four_pass = 1;
      c2.max_parts = fb->max_parts;
      dspsr_amd_filterbank* inv = nullptr;
      if (dspsr_amd_filterbank_create(fb->ctx, &c2, &inv) == DSPSR_AMD_OK && inv) {
        if (inv->g.four_pass && !inv->g.xblocked && inv->p3a.kern && inv->p3b.kern && inv->g.logMf == g.logMf) fb->batch = inv;
        else dspsr_amd_filterbank_destroy(inv);
      }
      fb->ctx->error[0] = 0;                   // (a refusal of the group object is not an error of this call)
    }
  }
}

// frees the device buffers and the object (create's failures come here directly: nothing of theirs was launched)
static void fb_release(dspsr_amd_filterbank* fb)
{
  for (void* p : {(void*)fb->A, (void*)fb->X, (void*)fb->kernel, (void*)fb->rmatrix, (void*)fb->kernel_nat, (void*)fb->S1, (void*)fb->S2, (void*)fb->Rt,
                  (void*)fb->det, (void*)fb->fpart, (void*)fb->msum, (void*)fb->dsub, (void*)fb->Xp, (void*)fb->Y, (void*)fb->tw_lo,
                  (void*)fb->tw_lo_m})
    if (p) (void)hipFree(p);
  delete fb;
}

extern "C" int dspsr_amd_filterbank_create(dspsr_amd_ctx* ctx, const dspsr_amd_filterbank_config* cfg,
                                           dspsr_amd_filterbank** out)
{
  if (!ctx || !cfg || !out) return DSPSR_AMD_EINVAL;
  *out = nullptr;
  if (cfg->npol != 1 && cfg->npol != 2)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_create: npol=%u not 1 or 2", cfg->npol);
  if (cfg->freq_res == 1) return fb_create_plain(ctx, cfg, out);
  FbFactors f;
  int rc = fb_check_factors(ctx, cfg, &f);
  if (rc != DSPSR_AMD_OK) return rc;
  dspsr_amd_filterbank* fb = new dspsr_amd_filterbank;
  fb->ctx = ctx; fb->cfg = *cfg; fb->ncu = ctx->ncu;
  fb_init_geom(fb, f);
  if ((rc = fb_tile(fb)) == DSPSR_AMD_OK && (rc = fb_pick_kernels(fb)) == DSPSR_AMD_OK) {
    fb_setup_two_pass(fb);
    rc = fb_alloc_scratch(fb);
  }
  if (rc != DSPSR_AMD_OK) { fb_release(fb); return rc; }
  fb_setup_conv(fb);
  *out = fb;
  return DSPSR_AMD_OK;
}

extern "C" void dspsr_amd_filterbank_destroy(dspsr_amd_filterbank* fb)
{
  if (!fb) return;
  if (fb->batch) dspsr_amd_filterbank_destroy(fb->batch);
  (void)hipStreamSynchronize(fb->ctx->stream);
  fb_release(fb);
}

// set_kernel replaces a matrix response
static void fb_drop_matrix(dspsr_amd_filterbank* fb)
{
  if (fb->rmatrix) (void)hipFree(fb->rmatrix);
  fb->rmatrix = nullptr;
}

extern "C" int dspsr_amd_filterbank_set_kernel(dspsr_amd_filterbank* fb, const float* kernel_host, uint64_t ncomplex)
{
  if (!fb) return DSPSR_AMD_EINVAL;
  if (!kernel_host) {  // no response: plain filterbank
    if (fb->kernel) (void)hipFree(fb->kernel);
    fb->kernel = nullptr;
    fb_drop_matrix(fb);
    fb->kernel_set = true;
    return DSPSR_AMD_OK;
  }
  const uint64_t expect = (uint64_t)fb->cfg.input_nchan * fb->N;
  if (ncomplex != expect)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_set_kernel: kernel has %llu bins, expected %llu",
                   (unsigned long long)ncomplex, (unsigned long long)expect);
  if (!fb->kernel && hipMalloc((void**)&fb->kernel, expect * sizeof(cf)) != hipSuccess)
    return fb_fail(fb->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_set_kernel: hipMalloc failed");
  const cf* src = (const cf*)kernel_host;
  std::vector<cf> perm;
  if (fb->conv3_logM >= 0) {
    // the three-pass convolution reads the response in the order of its pass-B tiles (fb_conv3_response_order: whole lines per load)
    if (!fb->kernel_nat && hipMalloc((void**)&fb->kernel_nat, expect * sizeof(cf)) != hipSuccess)
      return fb_fail(fb->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_set_kernel: hipMalloc failed");
    std::vector<cf> ord(expect);
    for (uint32_t c = 0; c < fb->cfg.input_nchan; c++) fb_conv3_response_order(fb->conv3_logM, src + (uint64_t)c * fb->N, ord.data() + (uint64_t)c * fb->N);
    if (hipMemcpy(fb->kernel_nat, ord.data(), expect * sizeof(cf), hipMemcpyHostToDevice) != hipSuccess)
      return fb_fail(fb->ctx, DSPSR_AMD_EHIP, "dspsr_amd_filterbank_set_kernel: copy of the response failed");
  } else if (fb->conv1_logM >= 0 && fb->g.xblocked) {
    // (the one-pass convolution reads the response in natural order; the four-pass kernels of this geometry take it blocked)
    if (!fb->kernel_nat && hipMalloc((void**)&fb->kernel_nat, expect * sizeof(cf)) != hipSuccess)
      return fb_fail(fb->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_set_kernel: hipMalloc failed");
    if (hipMemcpy(fb->kernel_nat, src, expect * sizeof(cf), hipMemcpyHostToDevice) != hipSuccess)
      return fb_fail(fb->ctx, DSPSR_AMD_EHIP, "dspsr_amd_filterbank_set_kernel: copy of the response failed");
  }
  if (fb->g.xblocked) {
    // four-pass geometries: the chirp lies on the device in the order of the blocked spectrum (k_inv_a loads both alike)
    const FbGeom& g = fb->g;
    const uint64_t N = fb->N, maskA = (1ull << g.logM) - 1, maskT = (1ull << g.logT2) - 1;
    perm.resize(expect);
    for (uint64_t ic = 0; ic < fb->cfg.input_nchan; ic++)
      for (uint64_t k = 0; k < N; k++) {
        const uint64_t ka = k & maskA, kb = k >> g.logM;
        perm[ic * N + (ka >> g.logT2) * g.kblock + ((kb << g.logT2) | (ka & maskT))] = src[ic * N + k];
      }
    src = perm.data();
  }
  if (fb->msub) {
    // the inner filterbank's channels are the pseudo-channels (c, r): bin m' of pseudo-channel c*R + r is bin R*m' + r of channel c
    const uint64_t N = fb->N, R = fb->msub, Mo = fb->out_M, Mi = Mo / R;
    perm.resize(expect);
    for (uint64_t ic = 0; ic < fb->cfg.input_nchan; ic++)
      for (uint64_t k = 0; k < N; k++) {
        const uint64_t c = k / Mo, m = k - c * Mo, mi = m / R, r = m - mi * R;
        perm[ic * N + (c * R + r) * Mi + mi] = src[ic * N + k];
      }
    src = perm.data();
  }
  hipError_t e = hipMemcpyAsync(fb->kernel, src, expect * sizeof(cf), hipMemcpyHostToDevice, fb->ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(fb->ctx->stream);
  if (e != hipSuccess)
    return fb_fail(fb->ctx, DSPSR_AMD_EHIP, "dspsr_amd_filterbank_set_kernel: %s", hipGetErrorString(e));
  fb->kernel_set = true;
  fb_drop_matrix(fb);
  return DSPSR_AMD_OK;
}

// Matrix response (Response::operate(data1, data2), Response.C:515-585): the three-pass path of a power-of-two geometry only;
// every limit is checked before anything is allocated or changed
extern "C" int dspsr_amd_filterbank_set_response_matrix(dspsr_amd_filterbank* fb, const float* response_host, uint64_t nmatrix)
{
  if (!fb || !response_host) return DSPSR_AMD_EINVAL;
  const dspsr_amd_filterbank_config& c = fb->cfg;
  const char* fn = "dspsr_amd_filterbank_set_response_matrix";
  if (c.npol != 2)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: matrix convolution needs npol == 2 (npol=%u)", fn, c.npol);
  if (c.input_nchan != 1)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dsp::Filterbank::make_preparations matrix convolution untested for > one input channel "
                   "(input_nchan=%u)", c.input_nchan);
  if (c.freq_res < 2)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: the non-convolving filterbank (freq_res=%u) takes no matrix response: freq_res >= 2", fn,
                   c.freq_res);
  if (c.nchan_subband < 2)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: nchan_subband=%u (dsp::Convolution shapes) takes no matrix response: nchan_subband >= 2",
                   fn, c.nchan_subband);
  if (!ispow2(c.freq_res) || !ispow2(c.nchan_subband))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: nchan_subband=%u and freq_res=%u must be powers of two (no odd factor) for a matrix "
                   "response", fn, c.nchan_subband, c.freq_res);
  if (c.force_four_pass == 1)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: force_four_pass=1: the four-pass inverse takes no matrix response", fn);
  if (fb->g.four_pass || c.freq_res > 8192)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: freq_res=%u > 8192 (the four-pass inverse) takes no matrix response", fn, c.freq_res);
  if (nmatrix != fb->N)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: response has %llu matrices, expected nchan_subband*freq_res = %llu", fn,
                   (unsigned long long)nmatrix, (unsigned long long)fb->N);
  if (!fb->p3m.kern) {
    const FbGeom& g = fb->g;
    FbPass<k3_t> pm = fb->p3m;
    pm.kern = fb_pick3m(g.logM, g.logT3 + 1 == full_logt(g.logM), fb->presplit);
    if (!pm.kern) return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: no kernel for this geometry", fn);
    const hipError_t e = allow_lds(pm);
    if (e != hipSuccess) return fb_fail(fb->ctx, DSPSR_AMD_EHIP, "%s: hipFuncSetAttribute: %s", fn, hipGetErrorString(e));
    fb->p3m = pm;
  }
  const size_t bytes = (size_t)fb->N * 2 * sizeof(float4);
  float4* dev = fb->rmatrix;
  if (!dev && hipMalloc((void**)&dev, bytes) != hipSuccess)
    return fb_fail(fb->ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc of %zu response bytes failed", fn, bytes);
  // (the device image is the host array: bin k's eight floats are its two 16-byte halves)
  hipError_t e = hipMemcpyAsync(dev, response_host, bytes, hipMemcpyHostToDevice, fb->ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(fb->ctx->stream);
  if (e != hipSuccess) {
    if (!fb->rmatrix) (void)hipFree(dev);
    return fb_fail(fb->ctx, DSPSR_AMD_EHIP, "%s: %s", fn, hipGetErrorString(e));
  }
  fb->rmatrix = dev;
  if (fb->kernel) (void)hipFree(fb->kernel);
  fb->kernel = nullptr;
  fb->kernel_set = true;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_filterbank_response_ndim(const dspsr_amd_filterbank* fb)
{
  return !fb || !fb->kernel_set ? 0 : fb->rmatrix ? 8 : fb->kernel ? 2 : 0;
}

extern "C" int dspsr_amd_filterbank_sizes(const dspsr_amd_filterbank* fb, uint64_t* nsamp_fft,
                                          uint64_t* nsamp_overlap, uint64_t* nsamp_step, uint32_t* nkeep)
{
  if (!fb) return DSPSR_AMD_EINVAL;
  const uint64_t nfilt_tot = fb->cfg.nfilt_pos + fb->cfg.nfilt_neg;
  const uint64_t fft = fb->cfg.real_input ? 2 * fb->N : fb->N;                          // Filterbank.C:139-148
  const uint64_t ovl = (fb->cfg.real_input ? 2 : 1) * nfilt_tot * fb->cfg.nchan_subband;
  if (nsamp_fft) *nsamp_fft = fft;
  if (nsamp_overlap) *nsamp_overlap = ovl;
  if (nsamp_step) *nsamp_step = fft - ovl;
  if (nkeep) *nkeep = fb->msub ? fb->out_nkeep : fb->g.nkeep;
  return DSPSR_AMD_OK;
}

static FbInKind raw_kind(int layout) { return layout == DSPSR_AMD_RAW_CASPSR ? FB_IN_CASPSR : layout == DSPSR_AMD_RAW_UWB16 ? FB_IN_UWB16 : FB_IN_GENERIC8; }

// ---- the output forms (fb_common.h FbOutKind): every field a builder does not name is zero ---------------------------------------
static FbOut fb_out(FbOutKind kind, float* base, uint64_t chan_stride, uint64_t pol_stride, int state, uint32_t ndim)
{
  FbOut o = {};
  o.kind = kind; o.base = base; o.chan_stride = chan_stride; o.pol_stride = pol_stride; o.state = state; o.ndim = ndim;
  return o;
}
// complex rows, or nothing without a base
static FbOut fb_out_rows(float* base, uint64_t chan_stride, uint64_t pol_stride, uint64_t part_step)
{
  FbOut o = fb_out(base ? FB_OUT_COMPLEX : FB_OUT_NONE, base, chan_stride, pol_stride, 0, 2);
  o.part_step = part_step;
  return o;
}
static FbOut fb_out_detected(float* base, uint64_t chan_stride, uint64_t pol_stride, int state, uint32_t ndim)
{
  return fb_out(FB_OUT_DETECTED, base, chan_stride, pol_stride, state, ndim);
}
// fused fold into the profile of `fold`: one float4 per bin, or (planes2) the two float2 rows (PP, QQ) and (Re, Im) per channel
static FbOut fb_out_fold(dspsr_amd_fold* fold, int state, bool planes2, const uint32_t* pstart, const Interval* piv, uint32_t nparts)
{
  FbOut o = fb_out(FB_OUT_FOLD, fold->profile, 0, 0, state, 4);
  o.nbin = fold->nbin; o.nchan_prof = fold->nchan; o.prof_planes = planes2 ? 2u : 1u; o.plane_stride = fold->span;
  o.prof_span4 = planes2 ? fold->span / 2 : fold->span / 4;    // (float4 from one channel to the next: both rows of the channel, or one)
  o.fold = fold; o.pstart = pstart; o.piv = piv; o.nparts_plan = nparts;
  return o;
}
static bool fb_state_square_law(int state) { return state == DSPSR_AMD_INTENSITY || state == DSPSR_AMD_PPQQ; }
// fused fold of a square-law state (k_inv_chan<., 3 | 7, .>) into the profile of `fold`, npol npo x ndim 1: scalar accumulators, row
// (chan, q) at base + (chan * npo + q) * chan_stride -- the row span travels in the field the float4 form does not use
static FbOut fb_out_fold_sq(dspsr_amd_fold* fold, int state, uint32_t npo, const uint32_t* pstart, const Interval* piv, uint32_t nparts)
{
  FbOut o = fb_out(FB_OUT_FOLD, fold->profile, fold->span, 0, state, 1);
  o.nbin = fold->nbin; o.nchan_prof = fold->nchan; o.prof_planes = npo;
  o.fold = fold; o.pstart = pstart; o.piv = piv; o.nparts_plan = nparts;
  return o;
}
// segment sums of a block of nparts parts into msum: the fold form of a one-plane profile, with the segment plan
static FbOut fb_out_segsum(float* msum, dspsr_amd_fold* fold, int state, const uint32_t* off, const Interval* siv, const uint32_t* blk_first,
                           const uint32_t* bin_start, uint32_t nparts)
{
  FbOut o = fb_out_fold(fold, state, false, off, siv, nparts);
  o.kind = FB_OUT_SEGSUM; o.base = msum; o.blk_first = blk_first; o.bin_start = bin_start;
  return o;
}
static FbOut fb_out_search(float* base, uint64_t chan_stride, uint64_t pol_stride, int state, uint32_t tscrunch, uint32_t phase0, uint32_t G,
                           float* carry)
{
  FbOut o = fb_out(FB_OUT_SEARCH, base, chan_stride, pol_stride, state, 1);
  o.ts_sf = tscrunch; o.ts_phase0 = phase0; o.ts_G = G; o.ts_carry = carry;
  // (tscrunch 1: 2^32 does not fit -- t / 1 = t is the special case of ts_stage)
  o.ts_magic = tscrunch == 1 ? 0xffffffffu : (uint32_t)(((1ull << 32) + tscrunch - 1) / tscrunch);
  return o;
}
// the forms every path has: complex or detected rows (or nothing) from the last pass
static bool fb_out_is_rows(const FbOut& out) { return out.kind == FB_OUT_NONE || out.kind == FB_OUT_COMPLEX || out.kind == FB_OUT_DETECTED; }

// ---- launches ----------------------------------------------------------------------------------------------------------------------
static uint32_t grid_for(uint64_t items, uint32_t ncu)
{
  uint64_t gsz = items < ncu ? items : ncu;
  if (gsz >= 8) gsz &= ~7ull;
  return (uint32_t)gsz;
}
// one pass on `grid` workgroups, on the object's stream
template <class K, class... A>
static void fb_launch_grid(const dspsr_amd_filterbank* fb, const FbPass<K>& p, uint32_t grid, const A&... args)
{
  hipLaunchKernelGGL(p.kern, dim3(grid), dim3(p.threads), p.lds, fb->ctx->stream, args...);
}
// ... as a persistent grid over `items` work items: the workgroups the chip holds, a multiple of 8 so that the XCD-aware item order applies
template <class K, class... A>
static void fb_launch(const dspsr_amd_filterbank* fb, const FbPass<K>& p, uint64_t items, const A&... args)
{
  fb_launch_grid(fb, p, grid_for(items, fb->ncu * p.wg_per_cu), args...);
}
// items of the inverse pass: a (tile of channels, part) each; search mode: one workgroup per tile walks the parts in order
static uint64_t fb_inverse_items(const FbOut& out, uint32_t tiles, uint32_t parts) { return out.kind == FB_OUT_SEARCH ? tiles : (uint64_t)tiles * parts; }

static int fb_launch_status(dspsr_amd_ctx* ctx)
{
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DSPSR_AMD_OK : fb_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_filterbank_perform: launch failed: %s", hipGetErrorString(e));
}

// the fold plan on its way to the device (fb_run_with_plan): the first kernel that reads it waits for it here, before its launch
static int fb_plan_ready(dspsr_amd_filterbank* fb, dspsr_amd_fold* fold)
{
  if (!fb->plan_wait) return DSPSR_AMD_OK;
  const int rc = fold_plan_wait(fold, fb->plan_wait);
  fb->plan_wait = nullptr;
  return rc;
}

// whether a call's fused fold is the segmented one
static bool fb_fold_segmented(const dspsr_amd_filterbank* fb, const FbOut& out)
{
  return out.kind == FB_OUT_FOLD && dspsr_amd_filterbank_fold_is_fused_state(fb, out.state) == 2;
}

// Fused inverse pass of one launch (ns parts starting at part0).  With fewer channel tiles than compute units the parts
// are cut into runs folded by different workgroups (k_inv_chan, "Segmented"): partial profiles zeroed before, added to the
// profile in run order after the launch.  Not segmented: one workgroup owns a tile for all parts (exact time order).
static int fb_launch_fused(dspsr_amd_filterbank* fb, const FbPass<k3_t>& p3, const cf* X, const cf* kern, FbOut co, uint64_t part0,
                           uint32_t ns, bool two_pass = false)
{
  dspsr_amd_ctx* ctx = fb->ctx;
  const FbGeom& g = fb->g;
  // (two-pass path: the tile is Fb = 2^logFb2 channels)
  const uint32_t tiles = two_pass ? g.C >> g.logFb2 : g.C >> g.logT3, wgs = fb->ncu * p3.wg_per_cu;
  uint32_t nseg = 1;
  if (fb_fold_segmented(fb, co) && tiles < wgs) {
    nseg = wgs / tiles;
    if (nseg > ns) nseg = ns;
    if (nseg > 16) nseg = 16;
    if (nseg < 1) nseg = 1;
  }
  const int rc = fb_plan_ready(fb, co.fold);
  if (rc != DSPSR_AMD_OK) return rc;
  co.plan_cap = two_pass ? fb->plan_cap2 : fb->plan_cap;
  co.nseg = nseg;
  co.part = nullptr;
  if (nseg > 1) {
    // (floats per bin of a channel: the float4, or the npo rows of a square-law state, packed [seg-1][chan][npo][nbin])
    const size_t need = (size_t)(nseg - 1) * g.C * co.nbin * (fb_state_square_law(co.state) ? co.prof_planes : 4u);
    if (!grow_device_buffer(ctx->stream, fb->fpart, fb->fpart_floats, need))
      return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform_fold: hipMalloc of %zu partial-profile bytes failed",
                     need * sizeof(float));
    if (hipMemsetAsync(fb->fpart, 0, need * sizeof(float), ctx->stream) != hipSuccess)
      return fb_fail(ctx, DSPSR_AMD_EHIP, "dspsr_amd_filterbank_perform_fold: hipMemsetAsync failed");
    co.part = fb->fpart;
  }
  if (nseg == 1) {
    fb_launch(fb, p3, tiles, g, X, kern, co, ctx->tw, part0, ns, ns);
    return DSPSR_AMD_OK;
  }
  fb_launch_grid(fb, p3, tiles * nseg, g, X, kern, co, ctx->tw, part0, ns, ns);      // (a workgroup per tile and run)
  return fold_combine_partials(co.fold, "fused fold: combine", fb->fpart, nseg - 1, co.chan0, g.C);
}

// output channels per input channel / kept samples per part as the caller sees them (freq_res = 3 * 2^k / 5 * 2^k: g describes the
// inner filterbank of pseudo-channels)
static inline uint32_t fb_out_C(const dspsr_amd_filterbank* fb) { return fb->msub ? fb->out_C : fb->g.C; }
static inline uint32_t fb_out_nkeep(const dspsr_amd_filterbank* fb) { return fb->msub ? fb->out_nkeep : fb->g.nkeep; }

// parts of the next launch group: at most max_parts, and few enough that every pass -- the forward passes of gf on nseq
// sequences per part, the inverse passes of gi -- stays below 2^31 work items (the kernels count them in 32 bits)
static uint32_t fb_group_parts(uint64_t left, uint32_t max_parts, const FbGeom& gf, uint64_t nseq, const FbGeom& gi)
{
  uint64_t items = (uint64_t)((1u << gf.logR) >> gf.logT1) * nseq;
  for (const uint64_t i : {(uint64_t)((1u << gf.logM) >> gf.logT2) * nseq, gi.four_pass ? 0 : (uint64_t)(gi.C >> gi.logT3),
                           gi.four_pass ? ((uint64_t)gi.C << (gi.logMb - gi.logTm)) : 0, gi.four_pass ? ((uint64_t)gi.C << (gi.logMa - gi.logTt)) : 0})
    if (i > items) items = i;
  uint32_t nb = (uint32_t)(left < max_parts ? left : max_parts);
  while (nb > 1 && items * nb >= (1ull << 31)) nb /= 2;
  return nb;
}

// dsp::Convolution on the channels of a filterbank, one launch group per GROUP of channels (see fb_setup_conv):
//   pass 1 / pass 2   this object's kernels and per-channel geometry on the virtual sequences vp = (part * 2 + pol) * CH + c of the
//                     group (FbIn::batch): spectra X[vp][freq_res] = X[part][pol][c][m], natural order
//   inverse passes    those of the group object (CH channels per "input channel", four-pass, natural order): its X layout is exactly
//                     that, its chirp slice [CH][freq_res] the group's rows of this object's kernel, its output channels chan0 + c
// Same kernels, same arithmetic per channel as the loop over the channels.
static int fb_run_batched(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride)
{
  dspsr_amd_ctx* ctx = fb->ctx;
  dspsr_amd_filterbank* inv = fb->batch;
  const FbGeom& gf = fb->g;
  const FbGeom& gi = inv->g;
  const uint32_t CH = inv->cfg.nchan_subband, ngroup = fb->cfg.input_nchan / CH;
  const uint32_t Rr = 1u << gf.logR, M = 1u << gf.logM;
  const float* in_f32 = (const float*)in.base;
  for (uint32_t grp = 0; grp < ngroup; grp++) {
    const cf* kern = fb->kernel ? fb->kernel + (uint64_t)grp * CH * fb->N : nullptr;
    FbOut co = out;
    co.chan0 = grp * CH;
    uint32_t nb = 0;
    for (uint64_t part0 = 0; part0 < npart; part0 += nb) {
      nb = fb_group_parts(npart - part0, inv->max_parts, gf, 2 * CH, gi);
      const uint32_t nvp = nb * 2 * CH;
      FbIn ci = in;
      ci.base = in_f32 + (uint64_t)grp * CH * chan_stride;
      ci.batch = CH;
      ci.chan_stride_c = chan_stride / 2;
      ci.nchan = 1; ci.ichan = 0;
      const uint64_t n1 = (uint64_t)(Rr >> gf.logT1) * nvp, n2 = (uint64_t)(M >> gf.logT2) * nvp;
      fb_launch(fb, fb->p1_w4, n1, gf, ci, inv->A, ctx->tw, part0, nvp, 1u, 32u);
      fb_launch(fb, fb->p2, n2, gf, inv->A, inv->X, ctx->tw, nvp, 1u, 4u);
      const uint64_t n3a = ((uint64_t)gi.C << (gi.logMb - gi.logTm)) * nb, n3b = ((uint64_t)gi.C << (gi.logMa - gi.logTt)) * nb;
      fb_launch(fb, inv->p3a, n3a, gi, inv->X, kern, inv->A, ctx->tw, nb, 8u);
      fb_launch(fb, inv->p3b, n3b, gi, inv->A, co, ctx->tw, part0, nb, 8u);
    }
  }
  return fb_launch_status(ctx);
}

// the non-convolving filterbank (fb_plain.hip): one launch per call
static int fb_run_plain(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride)
{
  if (!fb_out_is_rows(out))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform: output kind %d has no non-convolving form", (int)out.kind);
  const int rc = fb_plain_launch(fb->ctx, fb->plain_logC, fb->g.real_input != 0, (uint32_t)fb->g.npol, fb->cfg.input_nchan, fb->kernel, in,
                                 out, chan_stride, npart);
  return rc == DSPSR_AMD_OK ? rc : fb_fail(fb->ctx, rc, "dspsr_amd_filterbank_perform: launch of the non-convolving filterbank failed");
}

// the one-pass convolution (fb_conv1.hip)
static int fb_run_conv1(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride)
{
  const FbGeom& g = fb->g;
  const cf* kern = fb->kernel ? (g.xblocked ? fb->kernel_nat : fb->kernel) : nullptr;
  const Conv1Heaps heaps = {in.base, (uint32_t)in.part_step, in.heap_first, in.heap_swap != 0, in.scale};
  const int rc = in.kind == FB_IN_HEAPS
                     ? fb_conv1_launch(fb->ctx, fb->conv1_logM, nullptr, 0, 0, 0, &heaps, kern, out, fb->cfg.input_nchan, g.nfilt_pos, g.nkeep, npart)
                     : fb_conv1_launch(fb->ctx, fb->conv1_logM, (const float*)in.base, chan_stride, in.pol_stride, 2 * in.part_step, nullptr, kern,
                                       out, fb->cfg.input_nchan, g.nfilt_pos, g.nkeep, npart);
  return rc == DSPSR_AMD_OK ? rc : fb_fail(fb->ctx, rc, "dspsr_amd_filterbank_perform: launch of the one-pass convolution failed");
}

// the three-pass convolution (fb_conv3.hip): launch groups of conv3_ch channels x conv3_parts parts
static int fb_run_conv3(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride)
{
  dspsr_amd_ctx* ctx = fb->ctx;
  const FbGeom& g = fb->g;
  if (!fb->S1) {
    if (hipMalloc((void**)&fb->S1, fb->conv3_bytes) != hipSuccess || hipMalloc((void**)&fb->S2, fb->conv3_bytes) != hipSuccess) {
      if (fb->S1) (void)hipFree(fb->S1);
      fb->S1 = fb->S2 = nullptr;
      (void)hipGetLastError();
      return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform: hipMalloc of 2 x %llu bytes of scratch for the three-pass convolution failed",
                     (unsigned long long)fb->conv3_bytes);
    }
  }
  const cf* kern = fb->kernel ? fb->kernel_nat : nullptr;             // (in pass-B order, see set_kernel)
  for (uint32_t c0 = 0; c0 < fb->cfg.input_nchan; c0 += fb->conv3_ch) {
    const uint32_t nc = fb->cfg.input_nchan - c0 < fb->conv3_ch ? fb->cfg.input_nchan - c0 : fb->conv3_ch;
    FbOut co = out;
    co.chan0 = out.chan0 + c0;
    for (uint64_t part0 = 0; part0 < npart; part0 += fb->conv3_parts) {
      const uint32_t np = (uint32_t)(npart - part0 < fb->conv3_parts ? npart - part0 : fb->conv3_parts);
      const int rc = fb_conv3_launch(ctx, fb->conv3_logM, (const float*)in.base + (uint64_t)c0 * chan_stride,
                                     chan_stride, in.pol_stride, 2 * in.part_step, kern ? kern + (uint64_t)c0 * fb->N : nullptr, co,
                                     nc, g.nfilt_pos, g.nkeep, part0, np, fb->S1, fb->S2);
      if (rc != DSPSR_AMD_OK) return fb_fail(ctx, rc, "dspsr_amd_filterbank_perform: launch of the three-pass convolution failed");
    }
  }
  return DSPSR_AMD_OK;
}

// the two-pass path of short responses takes exactly this input form (and every output form; the four-pass segment sums never
// apply: freq_res <= 4096)
// (whole columns, Fa = 2^14: k_raw_cols also takes blocks of several input channels; Fa < 2^14 goes through k_raw_transpose)
static bool fb_takes_two_pass(const dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out)
{
  const FbGeom& g = fb->g;
  return fb->two_pass && !fb->rmatrix && in.kind == FB_IN_GENERIC8 && !g.real_input && g.npol == 2 && out.kind != FB_OUT_SEGSUM && (in.part_step % 4) == 0 &&
         (fb->p1c.kern ? ((uintptr_t)in.base % (fb->cfg.input_nchan == 1 ? 16 : 4)) == 0
                  : (fb->cfg.input_nchan == 1 && ((uintptr_t)in.base % 16) == 0));
}

// How pass 1 reads `in`: regrouped per tile first (8-bit pairs by k_raw_transpose into Rt, allocated on first use; float32 pairs
// by k_float_transpose) or in place, and its load width (raww 1: one word per sample pair, 4: generic).  two: the call takes the
// two-pass path.  sub: `in` is a sub-sequence of the sub-band path (k_sub_split's output: 16-byte aligned rows of one channel)
enum FbRegroup { FB_REGROUP_NONE, FB_REGROUP_RAW, FB_REGROUP_FLOAT };
struct FbPass1 { FbRegroup regroup; int raww; };
static int fb_pass1(dspsr_amd_filterbank* fb, const FbIn& in, uint64_t chan_stride, bool two, bool sub, FbPass1* p1)
{
  const FbGeom& g = fb->g;
  const uintptr_t base = (uintptr_t)in.base;
  // 8-bit real dual-pol single-channel input: one 32-bit word per sample pair; regroup it per tile first
  // (k_raw_transpose) unless the rows are already long enough or the layout preconditions fail
  const bool fast8 = (in.kind == FB_IN_GENERIC8 || in.kind == FB_IN_CASPSR) && g.real_input && g.npol == 2 && in.nchan == 1 && (base % 4) == 0;
  // complex dual-pol generic order: the same regroup per polarisation; pass 1 then reads (re, im) byte pairs exactly
  // like the (pol0, pol1) pairs of real input, one aligned word per two columns
  const bool fastc = in.kind == FB_IN_GENERIC8 && !g.real_input && g.npol == 2 && in.nchan == 1 && (base % 16) == 0 && (in.part_step % 4) == 0 &&
                     g.logR >= 3;
  bool raw = two || ((fast8 || fastc) && g.logR >= 2 && g.logT1 <= 5);   // rows of >= 128 B need no regrouping
  // (CASPSR blocks need a part step % 4 == 0; so do the sub-band path's 8-bit real sub-sequences, generic 8-bit real blocks in
  //  the other paths do not -- the two conditions differ and are kept as they are)
  if (raw && (in.kind == FB_IN_CASPSR || sub) && (in.part_step % 4) != 0) raw = false;
  // float32 rows (what Filterbank::Engine::perform is given): regrouped likewise, 8-byte elements
  const bool flt = in.kind == FB_IN_FLOAT && g.npol == 2 && g.logR >= 6 && g.logM >= 1 && g.logT1 >= 1 && g.logT1 <= 4 && (base % 16) == 0 &&
                   (in.part_step % 4) == 0 && (in.pol_stride % 4) == 0 && (chan_stride % 4) == 0;
  *p1 = {raw ? FB_REGROUP_RAW : flt ? FB_REGROUP_FLOAT : FB_REGROUP_NONE, (raw || (fast8 && in.kind == FB_IN_GENERIC8)) ? 1 : 4};
  if (raw && !fb->Rt && hipMalloc((void**)&fb->Rt, (size_t)fb->max_parts * fb->nseq * fb->L * sizeof(uint16_t)) != hipSuccess)
    return fb_fail(fb->ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform: hipMalloc of the 8-bit regroup buffer failed");
  return DSPSR_AMD_OK;
}

// the passes of the multi-pass paths that depend on the call: pass 1 for its load width, the (last) inverse pass for the output form
// and the response (kern nullptr where the geometry has none)
struct FbPassKernels { FbPass<k1_t> p1, p1d; FbPass<k3_t> p3; FbPass<k3b_t> p3b; };
static FbPassKernels fb_pass_kernels(const dspsr_amd_filterbank* fb, const FbPass1& p1, const FbOut& out)
{
  return {p1.raww == 1 ? fb->p1_w1 : fb->p1_w4, p1.raww == 1 ? fb->p1d_w1 : fb->p1d_w4,
          out.kind == FB_OUT_FOLD ? (fb_state_square_law(out.state) ? fb->p3q : fb->p3f) : out.kind == FB_OUT_SEARCH ? (out.state == DSPSR_AMD_COHERENCE ? fb->p3c : fb->p3s) : fb->rmatrix ? fb->p3m : fb->p3,
          out.kind == FB_OUT_SEGSUM ? fb->p3bf : fb->p3b};
}

// The loop of the multi-pass paths: the input channels one after the other, each in launch groups of at most max_parts parts;
// group(ci, co, kern, part0, nb) issues one launch group of channel ci.ichan.
template <typename F>
static int fb_each_group(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride, F&& group)
{
  const FbGeom& g = fb->g;
  for (uint32_t ichan = 0; ichan < fb->cfg.input_nchan; ichan++) {
    FbIn ci = in;
    if (in.kind == FB_IN_FLOAT) ci.base = (const float*)in.base + ichan * chan_stride;
    ci.ichan = ichan;
    ci.nchan = fb->cfg.input_nchan;
    FbOut co = out;
    co.chan0 = ichan * g.C;
    // (matrix response: input_nchan == 1; the inverse pass k3m reads the pointer as 32-byte bins)
    const cf* kern = fb->rmatrix ? (const cf*)fb->rmatrix : fb->kernel ? fb->kernel + (uint64_t)ichan * fb->N : nullptr;
    uint32_t nb = 0;
    for (uint64_t part0 = 0; part0 < npart; part0 += nb) {
      nb = fb_group_parts(npart - part0, fb->max_parts, g, fb->nseq, g);
      const int rc = group(ci, co, kern, part0, nb);
      if (rc != DSPSR_AMD_OK) return rc;
    }
  }
  return fb_launch_status(fb->ctx);
}

// One sub-group of a launch group of the sub-band path: nb parts part0, part0 + rp, part0 + 2 rp, ... of input channel ichan
static int fb_subband_group(dspsr_amd_filterbank* fb, const FbIn& in, uint32_t ichan, uint64_t chan_stride, const FbOut& co,
                            const cf* kern, const FbPass<k3_t>& p3, uint64_t part0, uint32_t nb, uint32_t rp)
{
  dspsr_amd_ctx* ctx = fb->ctx;
  const FbGeom& g = fb->g;
  const uint32_t R = g.nsub, ndim = g.real_input ? 1u : 2u, Rr = 1u << g.logR, M = 1u << g.logM;
  // (sub-groups: the parts do not follow each other -- every part is a window of its own in the de-interleaved block, L / R
  //  samples per sub-sequence, instead of one contiguous range that would cover the other sub-groups' samples as well)
  const uint64_t step = in.part_step * rp;                                         // (a multiple of R, like L)
  const uint64_t wlen = rp > 1 ? fb->L / R : ((uint64_t)(nb - 1) * step + fb->L) / R, nper = rp > 1 ? (uint64_t)nb * wlen : wlen;
  const size_t es = in.kind == FB_IN_FLOAT ? (size_t)g.npol * ndim * sizeof(float) : (size_t)g.npol * ndim;   // bytes per sample, all pols
  const size_t sub_stride = (nper * es + 15) & ~(size_t)15;
  if (!grow_device_buffer(ctx->stream, fb->dsub, fb->dsub_bytes, sub_stride * R))
    return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform: hipMalloc of %zu sub-sequence bytes failed", sub_stride * R);
  SubSplit sp = {in.kind, in.base, in.kind == FB_IN_FLOAT ? (uint64_t)ichan * chan_stride : 0, in.pol_stride,
                 fb->cfg.input_nchan, ichan, (uint32_t)g.npol, ndim, part0 * in.part_step, nper, R, sub_stride,
                 rp > 1 ? nb : 1u, wlen, step};
  fb_launch_sub_split(ctx->stream, sp, fb->dsub, fb->ncu);
  const uint64_t Ls = fb->L / R;
  for (uint32_t c = 0; c < R; c++) {
    FbIn cs = in;
    cs.kind = in.kind == FB_IN_FLOAT ? FB_IN_FLOAT : FB_IN_GENERIC8;    // (the split writes the generic byte order)
    cs.base = fb->dsub + (size_t)c * sub_stride;
    cs.pol_stride = in.kind == FB_IN_FLOAT ? nper * ndim : 0;
    cs.part_step = rp > 1 ? wlen : step / R;
    cs.nchan = 1; cs.ichan = 0;
    FbPass1 p1;
    const int rc = fb_pass1(fb, cs, 0, false, true, &p1);
    if (rc != DSPSR_AMD_OK) return rc;
    const FbPass<k1_t>& p1s = p1.raww == 1 ? fb->p1_w1 : fb->p1_w4;
    if (!p1s.kern) return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform: no kernel for this geometry");
    FbIn cr = cs;
    // (one window per part: the sub-groups' parts are windows of their own)
    const RtLayout lay = rt_layout_per_part(g.logM, g.logR, g.logT1, fb->nseq);
    if (p1.regroup == FB_REGROUP_RAW) {
      fb_launch_raw_transpose(ctx->stream, g, cs, fb->Rt, 0, nb, fb->nseq, lay);
      fb_set_rt(cr, FB_IN_RT_BYTES, fb->Rt, lay);
    } else if (p1.regroup == FB_REGROUP_FLOAT) {
      // (the float regroup buffer is the X scratch in the power-of-two path; X holds finished sub-spectra here: use Rt's
      //  place in A's idle upper half -- A needs nseq * L' of its nseq * L elements per part)
      cf* ft = fb->A + (size_t)nb * fb->nseq * Ls;
      fb_launch_float_transpose(dim3((Rr + FB_FT_COLS - 1) / FB_FT_COLS, (M + FB_FT_ROWS - 1) / FB_FT_ROWS, nb * fb->nseq), ctx->stream, g, cs, ft, 0);
      fb_set_rt(cr, FB_IN_RT_FLOAT, ft, lay);
    }
    const uint64_t n1s = (uint64_t)(Rr >> g.logT1) * fb->nseq * nb, n2s = (uint64_t)(M >> g.logT2) * fb->nseq * nb;
    fb_launch(fb, p1s, n1s, g, cr, fb->A, ctx->tw, 0ull, nb, fb->nseq, 32u);
    fb_launch(fb, fb->p2, n2s, g, fb->A, fb->X + c * Ls, ctx->tw, nb, fb->nseq, 4u);
  }
  const uint32_t tiles = g.C >> g.logT3;
  if (fb->msub) {
    // freq_res = R * 2^k: the spectrum in pseudo-channel order (second buffer), the inverse pass on the R * nchan_subband
    // pseudo-channels keeping whole transforms (complex rows into Y), then the radix-R step in time into the caller's output
    const uint64_t Mi = 1ull << g.logM, xe = (uint64_t)fb->max_parts * fb->nseq * fb->L,
                   ye = (uint64_t)g.C * g.npol * fb->max_parts * Mi;
    if (!fb->Xp && hipMalloc((void**)&fb->Xp, xe * sizeof(cf)) != hipSuccess)
      return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform: hipMalloc of the pseudo-channel spectrum failed");
    if (!fb->Y && hipMalloc((void**)&fb->Y, ye * sizeof(cf)) != hipSuccess)
      return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform: hipMalloc of the pseudo-channel time series failed");
    (void)fb_launch_sub_combine(ctx->stream, g, fb->X, nb * fb->nseq, fb->ncu, nullptr, fb->Xp, fb->out_M, fb->msub);
    // Y[pseudo-channel][pol][part of the group][Mi] complex: rows (pseudo-channel, pol), parts 2*Mi floats apart
    const FbOut yo = fb_out_rows((float*)fb->Y, (uint64_t)g.npol * fb->max_parts * Mi * 2, (uint64_t)fb->max_parts * Mi * 2, Mi * 2);
    fb_launch(fb, fb->p3, fb_inverse_items(yo, tiles, nb), g, fb->Xp, kern, yo, ctx->tw, 0ull, nb, nb);
    TimeCombine tc = {fb->Y, (uint64_t)g.npol * fb->max_parts * Mi, (uint64_t)fb->max_parts * Mi, (uint32_t)g.logM, fb->out_M,
                      fb->out_nfilt_pos, fb->out_nkeep, fb->out_C, (uint32_t)g.npol, part0, nb, rp, make_odd_tw(fb->msub)};
    FbOut cu = co;
    cu.chan0 = ichan * fb->out_C;
    if (cu.kind == FB_OUT_COMPLEX || cu.kind == FB_OUT_DETECTED) fb_launch_time_combine(ctx->stream, tc, cu, fb->msub, fb->ncu);
    return DSPSR_AMD_OK;
  }
  if (rp != 1) return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform: part step %llu is not a multiple of %u",
                              (unsigned long long)in.part_step, R);            // (cannot happen: see fb_run_subbands)
  // (factors without a radix kernel of their own combine out of place, into the A scratch -- idle behind pass 2)
  const cf* Xc = fb_launch_sub_combine(ctx->stream, g, fb->X, nb * fb->nseq, fb->ncu, fb->A);
  if (co.kind == FB_OUT_FOLD) return fb_launch_fused(fb, p3, Xc, kern, co, part0, nb);
  fb_launch(fb, p3, fb_inverse_items(co, tiles, nb), g, Xc, kern, co, ctx->tw, part0, nb, nb);
  return DSPSR_AMD_OK;
}

// nchan_subband = 3 * 2^k / 5 * 2^k: the group's samples as nsub interleaved sub-sequences, passes 0-2 on each (the
// power-of-two geometry), one radix-nsub step on the sub-spectra, then the inverse pass on nsub << logR rows; freq_res with
// an odd factor (msub) adds the radix-msub step in time (k_time_combine)
static int fb_run_subbands(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride,
                           const FbPass<k3_t>& p3)
{
  const uint32_t R = fb->g.nsub;
  if (in.kind == FB_IN_UWB16)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform: 16-bit UWB blocks need power-of-two nchan_subband and "
                   "freq_res (k_sub_split de-interleaves 8-bit and float32 input)");
  // The sub-sequences of a launch share ONE de-interleaved block, so its parts must start a multiple of R samples apart.  The
  // part step is a multiple of the odd factor of nchan_subband always, of the factor of freq_res only when the kept length
  // allows it: otherwise the group runs as rp interleaved sub-groups -- parts q, q + rp, q + 2 rp, ... start rp steps apart,
  // a multiple of R -- each with its own de-interleave (round 4 fell back to ONE part per launch here: a cliff for persistent
  // kernels that amortise ramp-up and tail over 32-256 parts).
  auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; };
  const uint32_t rp = (in.part_step % R) ? R / gcd((uint32_t)(in.part_step % R), R) : 1u;
  return fb_each_group(fb, in, out, npart, chan_stride, [&](const FbIn& ci, const FbOut& co, const cf* kern, uint64_t part0, uint32_t nb) {
    for (uint32_t q = 0; q < rp && q < nb; q++) {
      const int rc = fb_subband_group(fb, in, ci.ichan, chan_stride, co, kern, p3, part0 + q, (nb - q + rp - 1) / rp, rp);
      if (rc != DSPSR_AMD_OK) return rc;
    }
    return DSPSR_AMD_OK;
  });
}

// Two passes (fb_two_pass.hip): regroup per column, whole-column forward pass, rows + inverse pass -- the spectrum never
// leaves the chip.  Launches are whole groups (the segmented fused fold pays a memset and a combine pass per launch).
static int fb_run_two_pass(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride)
{
  dspsr_amd_ctx* ctx = fb->ctx;
  const FbGeom& g = fb->g;
  const uint32_t Fb = 1u << g.logFb2, tiles = g.C >> g.logFb2;
  return fb_each_group(fb, in, out, npart, chan_stride, [&](const FbIn& ci, const FbOut& co, const cf* kern, uint64_t part0, uint32_t nb) {
    FbIn cr = ci;
    cr.kind = FB_IN_RT_BYTES;
    cr.base = fb->Rt;
    if (fb->p1c.kern) {
      fb_launch_raw_cols(dim3((uint32_t)(fb->L / 8192), nb), ctx->stream, g, ci, fb->Rt, part0);
      fb_launch(fb, fb->p1c, (uint64_t)Fb * 2 * nb, g, cr, fb->A, ctx->tw, nb, 2u, 32u);
    } else {
      const FbGeom& q = fb->g1t;
      const RtLayout lay = rt_layout_per_part(q.logM, q.logR, q.logT1, 2);
      fb_launch_raw_transpose(ctx->stream, q, ci, fb->Rt, part0, nb, 2, lay);
      fb_set_rt(cr, FB_IN_RT_BYTES, fb->Rt, lay);
      fb_launch(fb, fb->p1t, (uint64_t)(Fb >> q.logT1) * 2 * nb, q, cr, fb->A, ctx->tw, part0, nb, 2u, 32u);
    }
    if (co.kind == FB_OUT_FOLD) return fb_launch_fused(fb, fb->p2rf, fb->A, kern, co, part0, nb, true);
    fb_launch(fb, co.kind == FB_OUT_SEARCH ? (co.state == DSPSR_AMD_COHERENCE ? fb->p2rc : fb->p2rs) : fb->p2r, fb_inverse_items(co, tiles, nb), g, fb->A, kern, co, ctx->tw, part0, nb, nb);
    return DSPSR_AMD_OK;
  });
}

// The three- and four-pass tile passes: pass 1 (after the regroup p1 chose), pass 2, then the inverse pass (three-pass: one,
// plain, fused fold or search; four-pass: two, the second one plain or leaving fold segment sums)
static int fb_run_tiles(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride,
                        const FbPass1& p1, const FbPassKernels& k)
{
  dspsr_amd_ctx* ctx = fb->ctx;
  const FbGeom& g = fb->g;
  const uint32_t Rr = 1u << g.logR, M = 1u << g.logM;
  return fb_each_group(fb, in, out, npart, chan_stride, [&](const FbIn& ci, const FbOut& co, const cf* kern, uint64_t part0, uint32_t nb) {
    const uint64_t n1 = (uint64_t)(Rr >> g.logT1) * fb->nseq * nb;
    const uint32_t tiles = g.C >> g.logT3;                            // (of the one inverse pass of the three-pass geometry)
    // XCD dealing of the persistent items (wgfft.h persistent_item): runs of consecutive items per XCD (the inverse pass: its parts)
    const uint32_t run1 = 32, run2 = 4;
    FbIn c1 = ci;
    RtLayout lay = rt_layout_per_part(g.logM, g.logR, g.logT1, fb->nseq);
    if (p1.regroup == FB_REGROUP_RAW) {
      // parts that start whole rows apart read their windows from ONE regrouped row grid: the rows neighbours share are
      // regrouped once (headline: 104908 rows instead of 131072 per 32 parts); never larger than the per-part image Rt is
      // allocated for (rt_takes_shared)
      if (rt_takes_shared(g.logM, g.logR, nb, ci.part_step)) lay = rt_layout_shared(g.logM, g.logR, g.logT1, nb, ci.part_step >> g.logR);
      fb_launch_raw_transpose(ctx->stream, g, ci, fb->Rt, part0, nb, fb->nseq, lay);
      fb_set_rt(c1, FB_IN_RT_BYTES, fb->Rt, lay);
    } else if (p1.regroup == FB_REGROUP_FLOAT) {
      // (into the idle X scratch)
      fb_launch_float_transpose(dim3((Rr + FB_FT_COLS - 1) / FB_FT_COLS, (M + FB_FT_ROWS - 1) / FB_FT_ROWS, nb * fb->nseq), ctx->stream, g, ci, fb->X, part0);
      fb_set_rt(c1, FB_IN_RT_FLOAT, fb->X, lay);
    }
    // (the dual pass takes pairs of tiles; run is a divisor in persistent_item: never 0)
    if (k.p1d.kern) fb_launch(fb, k.p1d, n1 / 2, g, c1, fb->A, ctx->tw, part0, nb, fb->nseq, run1 / 2 ? run1 / 2 : 1u);
    else fb_launch(fb, k.p1, n1, g, c1, fb->A, ctx->tw, part0, nb, fb->nseq, run1);
    // Pass 2 and the inverse pass run in sub-groups of a few parts, so that
    // part of the spectrum pass 2 has just written is still in the 256 MB Infinity Cache when the inverse pass reads
    // it (measured with whole groups of 8 / 16 / 32 parts: 31.5 / 33.4 / 35.2 µs per part in the inverse pass, pass 2
    // unchanged) while passes 0 and 1 keep the long launch their persistent workgroups want.
    // Sub-group = about 512 MB of spectrum (8 parts of the headline geometry; small geometries keep whole launches:
    // cut into 8 parts, -F 256:D loses 9 % and the 50 MHz sub-band geometry 24 %).
    uint64_t p23auto = (512ull << 20) / (fb->part_elems * sizeof(cf));
    if (p23auto < 1) p23auto = 1;
    // (the fused kernel gains less, +1.4 % Msamples/s measured in three alternating runs, but consistently)
    // (segmented fused fold -- geometries with fewer channel tiles than compute units: every launch of the fused kernel
    //  brings a memset and a combine pass over the partial profiles, so whole launches win: 50 MHz sub-band geometry
    //  43.5k -> 46.0k Msamples/s, -F 256:D 60.3k -> 60.6-61.3k, tools/exp_p23.sh)
    const uint32_t p23sub = (g.four_pass || fb_fold_segmented(fb, co)) ? nb : (uint32_t)(p23auto < nb ? p23auto : nb);
    for (uint32_t s0 = 0; s0 < nb; s0 += p23sub) {
      const uint32_t ns = nb - s0 < p23sub ? nb - s0 : p23sub;
      const uint64_t off = (uint64_t)s0 * fb->part_elems;
      fb_launch(fb, fb->p2, (uint64_t)(M >> g.logT2) * fb->nseq * ns, g, fb->A + off, fb->X + off, ctx->tw, ns, fb->nseq, run2);
      if (g.four_pass) break;                       // (the whole group: its two inverse passes follow)
      // fused fold: one workgroup owns a tile (T3 channels) for all parts of the launch
      if (co.kind == FB_OUT_FOLD) {
        const int rc = fb_launch_fused(fb, k.p3, fb->X + off, kern, co, part0 + s0, ns);
        if (rc != DSPSR_AMD_OK) return rc;
      } else {
        fb_launch(fb, k.p3, fb_inverse_items(co, tiles, ns), g, fb->X + off, kern, co, ctx->tw, part0 + s0, ns, ns);
      }
    }
    if (!g.four_pass) return DSPSR_AMD_OK;
    // two-pass inverse: X (whole spectrum) -> U (in the A buffer, dead after pass 2) -> output
    const uint64_t n3a = ((uint64_t)g.C << (g.logMb - g.logTm)) * nb, n3b = ((uint64_t)g.C << (g.logMa - g.logTt)) * nb;
    fb_launch(fb, fb->p3a, n3a, g, fb->X, kern, fb->A, ctx->tw, nb, 8u);
    if (co.kind == FB_OUT_SEGSUM) {      // the fused second pass reads the segment plan
      const int rc = fb_plan_ready(fb, co.fold);
      if (rc != DSPSR_AMD_OK) return rc;
    }
    fb_launch(fb, k.p3b, n3b, g, fb->A, co, ctx->tw, part0, nb, 8u);
    // every part of this sub-band has left its segment sums: add them to the profile in time order
    if (co.kind == FB_OUT_SEGSUM && part0 + nb == npart)
      return fold_segment_combine(co.fold, fb->msum, co.chan0, g.C, (uint32_t)npart, g.nkeep, g.nfilt_pos, g.logTt, g.logMa,
                                  g.logMb, co.bin_start, co.piv);
    return DSPSR_AMD_OK;
  });
}

// One filterbank call: the common checks, then the first path whose conditions the object and the call meet.
static int fb_run(dspsr_amd_filterbank* fb, const FbIn& in, const FbOut& out, uint64_t npart, uint64_t chan_stride)
{
  dspsr_amd_ctx* ctx = fb->ctx;
  const FbGeom& g = fb->g;
  if (!fb->kernel_set)
    return fb_fail(ctx, DSPSR_AMD_ESTATE, "dspsr_amd_filterbank_perform: set_kernel (Engine::setup) not called");
  if (npart == 0) return DSPSR_AMD_OK;
  // the CASPSR and UWB loaders read whole 16-bit / 32-bit words relative to the block (fetch_pair, k_fb_plain): a block that
  // starts inside such a word is not that layout
  if ((in.kind == FB_IN_CASPSR && ((uintptr_t)in.base % 2) != 0) || (in.kind == FB_IN_UWB16 && ((uintptr_t)in.base % 4) != 0))
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform: a %s block must start at a multiple of %d bytes",
                   in.kind == FB_IN_CASPSR ? "CASPSR" : "16-bit UWB", in.kind == FB_IN_CASPSR ? 2 : 4);
  if (fb->plain_logC >= 0) return fb_run_plain(fb, in, out, npart, chan_stride);
  // complex float32 rows that the one- and three-pass convolutions read in place: an 8-byte base and even strides
  const bool conv_rows = in.kind == FB_IN_FLOAT && fb_out_is_rows(out) && (chan_stride % 2) == 0 && (in.pol_stride % 2) == 0 &&
                         ((uintptr_t)in.base % 8) == 0;
  if (fb->conv1_logM >= 0 && conv_rows) return fb_run_conv1(fb, in, out, npart, chan_stride);
  // a block of heaps: the one-pass convolution's second loader and nothing else (fb_input has refused every other object)
  if (in.kind == FB_IN_HEAPS) {
    if (fb->conv1_logM < 0 || !fb_out_is_rows(out))
      return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform: output kind %d has no form that reads MeerKAT heaps", (int)out.kind);
    return fb_run_conv1(fb, in, out, npart, chan_stride);
  }
  if (fb->conv3_logM >= 0 && conv_rows) return fb_run_conv3(fb, in, out, npart, chan_stride);
  if (fb->batch && in.kind == FB_IN_FLOAT && fb_out_is_rows(out) && (chan_stride % 2) == 0)
    return fb_run_batched(fb, in, out, npart, chan_stride);
  // the multi-pass paths: pass 1's regroup of the caller's input (its buffer allocated here) and the kernels
  const bool two = fb_takes_two_pass(fb, in, out);
  FbPass1 p1;
  const int rc = fb_pass1(fb, in, chan_stride, two, false, &p1);
  if (rc != DSPSR_AMD_OK) return rc;
  const FbPassKernels k = fb_pass_kernels(fb, p1, out);
  // (set_response_matrix admits the three-pass path of a power-of-two geometry only; fold and search detour through the detected /
  //  complex rows)
  if (fb->rmatrix && (!fb_out_is_rows(out) || g.four_pass || g.nsub > 1 || fb->msub))
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform: output kind %d has no matrix-response form", (int)out.kind);
  if (!k.p1.kern || !fb->p2.kern || (g.four_pass ? (!fb->p3a.kern || !k.p3b.kern) : !k.p3.kern))
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform: no kernel for this geometry");
  if (g.nsub > 1) return fb_run_subbands(fb, in, out, npart, chan_stride, k.p3);
  if (two) return fb_run_two_pass(fb, in, out, npart, chan_stride);
  return fb_run_tiles(fb, in, out, npart, chan_stride, p1, k);
}

// The input of a perform call (`fn` names it in the messages): float32 rows in_step floats apart per part, or a raw block
// (raw_dev in raw_layout) whose parts are nsamp_step samples apart
static int fb_input(dspsr_amd_filterbank* fb, const char* fn, const float* in_f32_dev, uint64_t in_pol_stride, uint64_t in_step,
                    const int8_t* raw_dev, int raw_layout, float scale, FbIn* in)
{
  const dspsr_amd_filterbank_config& c = fb->cfg;
  if (in_f32_dev) {
    const uint32_t idim = c.real_input ? 1 : 2;
    if (in_step % idim)
      return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: in_step=%llu not a multiple of ndim", fn, (unsigned long long)in_step);
    *in = {FB_IN_FLOAT, 0, 0, in_f32_dev, in_pol_stride, in_step / idim, c.input_nchan, 0, 1.0f};
    return DSPSR_AMD_OK;
  }
  // a block of heaps: the layout word carries the index of the call's first sample inside the block's first heap
  const uint32_t first = raw_layout < 0 ? 0u : (uint32_t)raw_layout >> 8;
  if (first) raw_layout &= 0xff;
  const bool heaps = raw_layout == DSPSR_AMD_RAW_MEERKAT || raw_layout == DSPSR_AMD_RAW_MEERKAT_SWAP;
  if (first && !heaps)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: first_sample=%u on raw layout %d: only the heap layouts (DSPSR_AMD_RAW_MEERKAT, "
                   "DSPSR_AMD_RAW_MEERKAT_SWAP) carry one", fn, first, raw_layout);
  if (heaps) {
    if (first > 255)
      return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: first_sample=%u is not inside a heap of 256 samples", fn, first);
    if (fb->conv1_logM < 0)
      return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: this object does not read MeerKAT heaps (dspsr_amd_filterbank_takes_heaps() == 0: that "
                     "needs nchan_subband = 1, complex input, npol = 2, 64 <= freq_res <= 8192 and force_four_pass = 0; here nchan_subband=%u "
                     "real_input=%u npol=%u freq_res=%u force_four_pass=%u) -- dspsr_amd_unpack_heaps_fpt first, then the float32 entry points",
                     fn, c.nchan_subband, c.real_input, c.npol, c.freq_res, c.force_four_pass);
    if (((uintptr_t)raw_dev % 16) != 0)
      return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: a block of heaps must start at a multiple of 16 bytes", fn);
  }
  if (raw_layout == DSPSR_AMD_RAW_CASPSR && !(c.real_input && c.npol == 2 && c.input_nchan == 1))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: CASPSR layout needs real dual-pol single-channel input", fn);
  if (raw_layout == DSPSR_AMD_RAW_UWB16 && (c.real_input || c.input_nchan != 1))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: UWB 16-bit layout needs complex single-channel input", fn);
  if (raw_layout != DSPSR_AMD_RAW_CASPSR && raw_layout != DSPSR_AMD_RAW_GENERIC && raw_layout != DSPSR_AMD_RAW_UWB16 && !heaps)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: unknown raw layout %d", fn, raw_layout);
  uint64_t step;
  dspsr_amd_filterbank_sizes(fb, nullptr, nullptr, &step, nullptr);
  *in = {heaps ? FB_IN_HEAPS : raw_kind(raw_layout), (uint16_t)first, (uint16_t)(raw_layout == DSPSR_AMD_RAW_MEERKAT_SWAP), raw_dev, 0, step,
         c.input_nchan, 0, scale};
  return DSPSR_AMD_OK;
}

// perform / perform_raw (`fn` names the caller in the messages): the input, then the complex output rows -- a part's 2 * nkeep floats
// must fit its out_step, and the rows of different channels and polarisations must not overlap (a channel's row may not reach into the
// next channel's first polarisation either).  Any float-aligned address is taken: no writer needs more (tests/test_gpu_output_forms.py).
static int fb_perform_rows(dspsr_amd_filterbank* fb, const char* fn, const float* in_f32_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                           uint64_t in_step, const int8_t* raw_dev, int raw_layout, float scale, float* out_dev, uint64_t out_chan_stride,
                           uint64_t out_pol_stride, uint64_t npart, uint64_t out_step)
{
  FbIn in;
  const int rc = fb_input(fb, fn, in_f32_dev, in_pol_stride, in_step, raw_dev, raw_layout, scale, &in);
  if (rc != DSPSR_AMD_OK) return rc;
  if (out_dev && out_step < 2ull * fb_out_nkeep(fb))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: out_step=%llu < 2*nkeep=%u", fn, (unsigned long long)out_step, 2 * fb_out_nkeep(fb));
  const uint64_t nchan_out = (uint64_t)fb->cfg.input_nchan * fb_out_C(fb);
  const uint64_t row = npart ? (npart - 1) * out_step + 2ull * fb_out_nkeep(fb) : 0;      // floats one output row spans
  // channel-major (TimeSeries FPT order) or polarisation-major, as the detected rows of perform_detect
  if (out_dev && !fb_rows_ok(npart, nchan_out, fb->cfg.npol, out_chan_stride, out_pol_stride, row, true))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: output rows of %llu floats overlap (chan stride %llu, pol stride %llu)", fn,
                   (unsigned long long)row, (unsigned long long)out_chan_stride, (unsigned long long)out_pol_stride);
  return fb_run(fb, in, fb_out_rows(out_dev, out_chan_stride, out_pol_stride, out_step), npart, in_chan_stride);
}

extern "C" int dspsr_amd_filterbank_perform(dspsr_amd_filterbank* fb, const float* in_dev, uint64_t in_chan_stride,
                                            uint64_t in_pol_stride, float* out_dev, uint64_t out_chan_stride,
                                            uint64_t out_pol_stride, uint64_t npart, uint64_t in_step,
                                            uint64_t out_step)
{
  if (!fb || !in_dev) return DSPSR_AMD_EINVAL;
  return fb_perform_rows(fb, "dspsr_amd_filterbank_perform", in_dev, in_chan_stride, in_pol_stride, in_step, nullptr, 0, 0.0f, out_dev,
                         out_chan_stride, out_pol_stride, npart, out_step);
}

extern "C" int dspsr_amd_filterbank_perform_raw(dspsr_amd_filterbank* fb, const int8_t* raw_dev, int raw_layout,
                                                float scale, float* out_dev, uint64_t out_chan_stride,
                                                uint64_t out_pol_stride, uint64_t npart, uint64_t out_step)
{
  if (!fb || !raw_dev) return DSPSR_AMD_EINVAL;
  return fb_perform_rows(fb, "dspsr_amd_filterbank_perform_raw", nullptr, 0, 0, 0, raw_dev, raw_layout, scale, out_dev, out_chan_stride,
                         out_pol_stride, npart, out_step);
}

static int fb_detect_square_law(dspsr_amd_filterbank* fb, const char* fn, const FbIn& in, uint64_t in_chan_stride, int state, float** det,
                                uint64_t det_chan_stride, uint64_t det_pol_stride, uint64_t npart);      // (behind fb_search_fits)

extern "C" int dspsr_amd_filterbank_perform_detect(dspsr_amd_filterbank* fb, const float* in_f32_dev,
                                                   uint64_t in_chan_stride, uint64_t in_pol_stride, uint64_t in_step,
                                                   const int8_t* raw_dev, int raw_layout, float scale, int state,
                                                   uint32_t ndim, float* det_dev, uint64_t det_chan_stride,
                                                   uint64_t det_pol_stride, uint64_t npart)
{
  if (!fb || !det_dev || (!in_f32_dev == !raw_dev)) return DSPSR_AMD_EINVAL;
  if (fb_state_square_law(state)) {
    // Detection::square_law (dspsr -d 1, -d 2): rows [chan][npol_out] of npart * nkeep floats
    const char* fn = "dspsr_amd_filterbank_perform_detect";
    if (ndim != 1)
      return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: state=%d (%s) is detected with ndim=1, not ndim=%u", fn, state,
                     state == DSPSR_AMD_PPQQ ? "PPQQ" : "Intensity", ndim);
    if (state == DSPSR_AMD_PPQQ && fb->cfg.npol != 2)
      return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: PPQQ needs two polarisations (npol=%u)", fn, fb->cfg.npol);
    FbIn in;
    const int rc = fb_input(fb, fn, in_f32_dev, in_pol_stride, in_step, raw_dev, raw_layout, scale, &in);
    if (rc != DSPSR_AMD_OK) return rc;
    const uint64_t nchan_out = (uint64_t)fb->cfg.input_nchan * fb_out_C(fb), row = npart * fb_out_nkeep(fb);
    if (!fb_rows_ok(npart, nchan_out, state == DSPSR_AMD_PPQQ ? 2 : 1, det_chan_stride, det_pol_stride, row, true))
      return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "%s: detected rows of %llu floats overlap (chan stride %llu, pol stride %llu)", fn,
                     (unsigned long long)row, (unsigned long long)det_chan_stride, (unsigned long long)det_pol_stride);
    float* det = det_dev;
    return fb_detect_square_law(fb, fn, in, in_chan_stride, state, &det, det_chan_stride, det_pol_stride, npart);
  }
  if (fb->cfg.npol != 2)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL,
                   "dspsr_amd_filterbank_perform_detect: Cannot detect polarization when npol != 2");
  if (ndim != 1 && ndim != 2 && ndim != 4)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_detect: invalid ndim=%u", ndim);
  if (state != DSPSR_AMD_COHERENCE && state != DSPSR_AMD_STOKES)
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_detect: invalid state=%d", state);
  FbIn in;
  const int rc = fb_input(fb, "dspsr_amd_filterbank_perform_detect", in_f32_dev, in_pol_stride, in_step, raw_dev, raw_layout, scale, &in);
  if (rc != DSPSR_AMD_OK) return rc;
  // rows must not overlap: channel-major (TimeSeries FPT order) or plane-major layouts are accepted
  const uint64_t nchan_out = (uint64_t)fb->cfg.input_nchan * fb_out_C(fb), row = npart * fb_out_nkeep(fb) * ndim, planes = 4 / ndim;
  if (!fb_rows_ok(npart, nchan_out, planes, det_chan_stride, det_pol_stride, row, true))
    return fb_fail(fb->ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_detect: detected rows of %llu floats overlap "
                   "(chan stride %llu, pol stride %llu)", (unsigned long long)row, (unsigned long long)det_chan_stride,
                   (unsigned long long)det_pol_stride);
  return fb_run(fb, in, fb_out_detected(det_dev, det_chan_stride, det_pol_stride, state, ndim), npart, in_chan_stride);
}

// search mode inside the inverse pass: the staged tile (fb_common.h ts_stage) must fit the exchange buffer and the 32-bit index
// arithmetic of the epilogue must hold
static bool fb_search_fits(const dspsr_amd_filterbank* fb, uint32_t npo, uint32_t sf, uint32_t* G_out)
{
  const FbGeom& g = fb->g;
  if (g.four_pass || fb->msub || fb->rmatrix || !fb->p3s.kern || g.nkeep >= 65536 || sf >= 32768) return false;
  const uint64_t ngmax = ((uint64_t)g.nkeep + 2ull * sf - 2) / sf;
  const uint32_t G = (uint32_t)ngmax | 1u;
  const uint64_t floats = ((uint64_t)npo << g.logT3) * sf * G;
  if (floats > 2ull * fb->p3s.threads * PTS) return false;                       // (the buffer's padding is slack)
  if (((uint64_t)npo << g.logT3) > 4ull * fb->p3s.threads) return false;         // a thread reads at most four rows' carries (k_inv_chan TS_NPRE)
  if (npo == 4) {
    // the Coherence form (k_inv_chan<., 18 | 22, .>, k_rows_inv<., ., 4>): four floats per (channel, sample) in the tile two floats
    // per (channel, polarisation, sample) came from, so `floats` above is the condition tscrunch * G <= freq_res; and the carries a
    // thread pre-loads are TS_NPRE of ITS kernel -- four where the transform has one stage (freq_res <= 16: both fuse, freq_res 8
    // is refused by the line above), two at freq_res 32 (two stages), one from freq_res 64 on
    if (!fb->p3c.kern) return false;
    const uint32_t npre = g.logM <= 4 ? 4 : g.logM == 5 ? 2 : 1;
    if (((uint64_t)npo << g.logT3) > (uint64_t)npre * fb->p3c.threads) return false;
  }
  if (((uint64_t)g.nkeep + sf) * sf >= (1ull << 32)) return false;       // t / sf by multiplication (ts_magic)
  if (G_out) *G_out = G;
  return true;
}

extern "C" int dspsr_amd_filterbank_search_is_fused(const dspsr_amd_filterbank* fb)
{
  return fb && fb_search_fits(fb, 2, 1, nullptr) ? 1 : 0;
}

// rows per channel of a search-mode state (0: not one)
static uint32_t fb_search_npol_out(int state)
{
  return state == DSPSR_AMD_INTENSITY ? 1u : state == DSPSR_AMD_PPQQ ? 2u : state == DSPSR_AMD_COHERENCE ? 4u : 0u;
}

extern "C" int dspsr_amd_filterbank_search_is_fused_state(const dspsr_amd_filterbank* fb, int out_state, uint32_t tscrunch)
{
  const uint32_t npo = fb_search_npol_out(out_state);
  if (!fb || !npo || !tscrunch || (npo != 1 && fb->cfg.npol != 2)) return 0;
  return fb_search_fits(fb, npo, tscrunch, nullptr) ? 1 : 0;
}

// Detection::square_law of a call at the filterbank's own rate (perform_detect, and the Detection of perform_fold's separate
// launches, with DSPSR_AMD_INTENSITY | DSPSR_AMD_PPQQ): rows [chan][npol_out] of npart * nkeep floats at *det + chan *
// det_chan_stride + q * det_pol_stride.  *det == nullptr: the rows go, packed, to the object's own block and *det is set.
// Where the search epilogue fits it runs with a scrunch factor of 1 -- it then writes the detected samples themselves and neither
// reads nor writes a carry -- else the complex rows go to the object's block and dspsr_amd_detect_square_law detects them: the
// two routes of perform_search, the same bits.
// floats from one row to the next of the detected rows the object keeps for itself: ndat rounded up to whole float4
static inline uint64_t fb_sq_own_row(uint64_t ndat) { return (ndat + 3) & ~3ull; }
static int fb_detect_square_law(dspsr_amd_filterbank* fb, const char* fn, const FbIn& in, uint64_t in_chan_stride, int state, float** det,
                                uint64_t det_chan_stride, uint64_t det_pol_stride, uint64_t npart)
{
  dspsr_amd_ctx* ctx = fb->ctx;
  const uint32_t npo = state == DSPSR_AMD_PPQQ ? 2u : 1u, npol = fb->cfg.npol;
  const uint64_t nchan_out = (uint64_t)fb->cfg.input_nchan * fb_out_C(fb), ndat = npart * fb_out_nkeep(fb);
  if (!ndat) return DSPSR_AMD_OK;
  uint32_t G = 0;
  const bool fused = ndat + 1 < (1ull << 32) && fb_search_fits(fb, npo, 1, &G);          // (the epilogue's 32-bit sample index)
  const uint64_t crow = 2 * ndat;
  const size_t ncplx = fused ? 0 : ((size_t)nchan_out * npol * crow + 3) & ~(size_t)3, nown = *det ? 0 : (size_t)nchan_out * npo * fb_sq_own_row(ndat);
  if (ncplx + nown && !grow_device_buffer(ctx->stream, fb->det, fb->det_floats, ncplx + nown))
    return fb_fail(ctx, DSPSR_AMD_ENOMEM, "%s: hipMalloc of %zu bytes failed", fn, (ncplx + nown) * sizeof(float));
  if (!*det) {                             // (16-byte aligned rows: the stand-alone fold's chunk kernels take them)
    *det = fb->det + ncplx;
    det_chan_stride = npo * fb_sq_own_row(ndat);
    det_pol_stride = fb_sq_own_row(ndat);
  }
  if (fused) return fb_run(fb, in, fb_out_search(*det, det_chan_stride, det_pol_stride, state, 1, 0, G, nullptr), npart, in_chan_stride);
  int rc = fb_run(fb, in, fb_out_rows(fb->det, npol * crow, crow, 2ull * fb_out_nkeep(fb)), npart, in_chan_stride);
  if (rc != DSPSR_AMD_OK) return rc;
  return dspsr_amd_detect_square_law(ctx, state == DSPSR_AMD_INTENSITY, fb->det, npol * crow, crow, *det, det_chan_stride, det_pol_stride,
                                     (uint32_t)nchan_out, npol, ndat);
}

extern "C" int dspsr_amd_filterbank_perform_search(dspsr_amd_filterbank* fb, const float* in_f32_dev, uint64_t in_chan_stride,
                                                   uint64_t in_pol_stride, uint64_t in_step, const int8_t* raw_dev, int raw_layout,
                                                   float scale, int out_state, uint32_t tscrunch, float* out_dev, uint64_t out_chan_stride,
                                                   uint64_t out_pol_stride, float* carry_dev, uint32_t* carry_count, uint64_t npart,
                                                   uint64_t* nout)
{
  if (!fb || (!in_f32_dev == !raw_dev) || !carry_count || !nout) return DSPSR_AMD_EINVAL;
  dspsr_amd_ctx* ctx = fb->ctx;
  if (out_state == DSPSR_AMD_STOKES)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_search: out_state=%d (Stokes) is not a search-mode state: Intensity, PPQQ "
                   "or Coherence", out_state);
  if (out_state != DSPSR_AMD_INTENSITY && out_state != DSPSR_AMD_PPQQ && out_state != DSPSR_AMD_COHERENCE)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_search: out_state=%d is neither Intensity, PPQQ nor Coherence", out_state);
  if (out_state == DSPSR_AMD_PPQQ && fb->cfg.npol != 2)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_search: PPQQ needs two polarisations (npol=%u)", fb->cfg.npol);
  if (out_state == DSPSR_AMD_COHERENCE && fb->cfg.npol != 2)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_search: Coherence needs two polarisations (npol=%u)", fb->cfg.npol);
  if (!tscrunch) return fb_fail(ctx, DSPSR_AMD_EINVAL, "dsp::TScrunch::get_factor scrunch factor not set");
  if (*carry_count >= tscrunch)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_search: carry_count=%u must be < tscrunch=%u", *carry_count, tscrunch);
  const uint32_t npo = fb_search_npol_out(out_state), nkeep = fb_out_nkeep(fb);
  const uint64_t ndat = npart * nkeep, total = (uint64_t)*carry_count + ndat;
  if (total + tscrunch >= (1ull << 32))
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_search: %llu parts x %u samples exceed the 32-bit sample index of a call",
                   (unsigned long long)npart, nkeep);
  const uint64_t no = total / tscrunch;                     // (*nout is written once the call is accepted: a refusal leaves it alone)
  const uint32_t rem = (uint32_t)(total % tscrunch);
  if (!npart) { *nout = no; return DSPSR_AMD_OK; }
  if ((!out_dev && no) || !carry_dev) return DSPSR_AMD_EINVAL;
  const uint64_t nchan_out = (uint64_t)fb->cfg.input_nchan * fb_out_C(fb);
  if (!fb_rows_ok(no, nchan_out, npo, out_chan_stride, out_pol_stride, no, false))           // (FPT rows: channel-major only)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_search: output rows of %llu floats overlap (chan stride %llu, pol "
                   "stride %llu)", (unsigned long long)no, (unsigned long long)out_chan_stride, (unsigned long long)out_pol_stride);
  FbIn in;
  int rc = fb_input(fb, "dspsr_amd_filterbank_perform_search", in_f32_dev, in_pol_stride, in_step, raw_dev, raw_layout, scale, &in);
  if (rc != DSPSR_AMD_OK) return rc;
  *nout = no;
  uint32_t G = 0;
  if (fb_search_fits(fb, npo, tscrunch, &G)) {
    // Filterbank + Detection (square_law, or the Coherence products) + TScrunch in one launch group: the detected stream never reaches HBM
    const FbOut out = fb_out_search(out_dev, out_chan_stride, out_pol_stride, out_state, tscrunch, *carry_count, G, carry_dev);
    rc = fb_run(fb, in, out, npart, in_chan_stride);
    if (rc != DSPSR_AMD_OK) return rc;
    *carry_count = rem;
    return DSPSR_AMD_OK;
  }
  // Other geometries (freq_res > 8192, freq_res with an odd factor, tiles the staged samples do not fit): the three operations one
  // after the other on a block owned by the object -- complex rows [chan][pol], detected rows behind them
  const uint64_t crow = 2 * ndat, drow = ndat;
  if (out_state == DSPSR_AMD_COHERENCE) {
    // the four products as Detection writes them with ndim 1 (rows [chan][4] of ndat floats, in the object's block), then TScrunch
    const size_t need4 = (size_t)nchan_out * 4 * drow;
    if (!grow_device_buffer(ctx->stream, fb->det, fb->det_floats, need4))
      return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform_search: hipMalloc of %zu bytes failed", need4 * sizeof(float));
    rc = fb_run(fb, in, fb_out_detected(fb->det, 4 * drow, drow, DSPSR_AMD_COHERENCE, 1), npart, in_chan_stride);
    if (rc != DSPSR_AMD_OK) return rc;
    return dspsr_amd_tscrunch_fpt(ctx, fb->det, 4 * drow, drow, out_dev, out_chan_stride, out_pol_stride, (uint32_t)nchan_out, 4, 1, ndat,
                                  tscrunch, carry_dev, carry_count, nout);
  }
  const size_t need = (size_t)nchan_out * (fb->cfg.npol * crow + npo * drow);
  if (!grow_device_buffer(ctx->stream, fb->det, fb->det_floats, need))
    return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform_search: hipMalloc of %zu bytes failed", need * sizeof(float));
  float* cplx = fb->det;
  float* det = fb->det + (size_t)nchan_out * fb->cfg.npol * crow;
  rc = fb_run(fb, in, fb_out_rows(cplx, fb->cfg.npol * crow, crow, 2ull * nkeep), npart, in_chan_stride);
  if (rc != DSPSR_AMD_OK) return rc;
  rc = dspsr_amd_detect_square_law(ctx, out_state == DSPSR_AMD_INTENSITY, cplx, fb->cfg.npol * crow, crow, det, npo * drow, drow,
                                   (uint32_t)nchan_out, fb->cfg.npol, ndat);
  if (rc != DSPSR_AMD_OK) return rc;
  return dspsr_amd_tscrunch_fpt(ctx, det, npo * drow, drow, out_dev, out_chan_stride, out_pol_stride, (uint32_t)nchan_out, npo, 1, ndat,
                                tscrunch, carry_dev, carry_count, nout);
}

extern "C" int dspsr_amd_filterbank_presplit(const dspsr_amd_filterbank* fb) { return fb && fb->presplit ? 1 : 0; }

extern "C" int dspsr_amd_filterbank_takes_heaps(const dspsr_amd_filterbank* fb) { return fb && fb->conv1_logM >= 0 ? 1 : 0; }

extern "C" int dspsr_amd_filterbank_npass(const dspsr_amd_filterbank* fb, int raw_input)
{
  if (!fb) return 0;
  if (fb->plain_logC >= 0) return 1;
  if (fb->conv1_logM >= 0 && !raw_input) return 1;
  if (fb->conv3_logM >= 0 && !raw_input) return 3;
  if (fb->g.four_pass) return 4;
  return fb->two_pass && raw_input && !fb->rmatrix ? 2 : 3;
}

extern "C" int dspsr_amd_filterbank_fold_is_fused(const dspsr_amd_filterbank* fb)
{
  // (short responses of dsp::Convolution shapes: Detection inside the one-pass kernel, Fold as a launch of its own -- the segment-sum
  //  fold belongs to the four-pass kernels)
  if (fb && (fb->conv1_logM >= 0 || fb->conv3_logM >= 0)) return 0;     // (the three-pass convolution likewise: Detection in pass C, Fold behind it)
  if (fb && fb->rmatrix) return 0;                                      // (matrix response: no fused instantiation; Detection + Fold)
  if (!fb || fb->msub || fb->plain_logC >= 0) return 0;            // (freq_res = 3 * 2^k / 5 * 2^k: the last step is a pass of its own, k_time_combine)
  // (segment sums pay when most of the transform is kept: at -F 64:D -x 16384 only 1817 of 16384 samples are, the unfused pass
  //  writes just those, and the fused one measured 541 against 458 us per 8 parts)
  if (fb->g.four_pass)
    return fb->cfg.fused_fold != DSPSR_AMD_FUSED_NEVER && fb->p3bf.kern && fb->g.logTt >= 3 &&
           (2ull * fb->g.nkeep >= (1ull << fb->g.logMf) || fb->cfg.fused_fold == DSPSR_AMD_FUSED_ALWAYS) ? 3 : 0;
  if (fb->g.nkeep >= 65536) return 0;
  if (fb->cfg.fused_fold == DSPSR_AMD_FUSED_ALWAYS) return 1;
  if (fb->cfg.fused_fold == DSPSR_AMD_FUSED_NEVER) return 0;
  // (a call that takes the two-pass path has the same tile count: Fb = 2^13 / freq_res channels per tile is the three-pass T3
  //  whenever nchan_subband >= Fb, which the two-pass path requires)
  const uint64_t tiles = (uint64_t)(fb->g.C >> fb->g.logT3);
  if (tiles >= fb->ncu) return 1;           // one workgroup per tile fills the chip: exact time-order sums
  return tiles >= 8 ? 2 : 0;                // fewer tiles: the parts of a launch are folded in runs (re-associated sums)
}

extern "C" int dspsr_amd_filterbank_fold_is_fused_state(const dspsr_amd_filterbank* fb, int state)
{
  const int mode = dspsr_amd_filterbank_fold_is_fused(fb);
  if (!fb_state_square_law(state)) return mode;
  // the square-law states: the three-pass kernel k_inv_chan<., 3 | 7, .> at the tile counts of the float4 fold -- measured at the
  // headline's freq_res with 8, 16, 32, 128 and 512 tiles, ms per 32 parts fused / Detection + Fold: Intensity 0.215 / 0.477, 0.223 /
  // 0.499, 0.233 / 0.542, 0.564 / 0.841, 2.098 / 2.436; PPQQ 0.216 / 0.618, 0.223 / 0.641, 0.234 / 0.681, 0.572 / 0.980, 2.077 /
  // 2.821 (profiles/fold_state_probe.txt): fused wins at every count, so none answers 0.  An object of one polarisation fuses
  // too (Intensity: the power of its polarisation).  No segment sums: the four-pass plan is not built for these states
  return (mode == 1 || mode == 2) && fb->p3q.kern ? mode : 0;
}

// fb_run with the fold plan in `slot` on its way to the device (no consumer launched: drained here), then handed back
static int fb_run_with_plan(dspsr_amd_filterbank* fb, dspsr_amd_fold* fold, PlanSlot* slot, const FbIn& in, const FbOut& out,
                            uint64_t npart, uint64_t chan_stride)
{
  fb->plan_wait = slot;
  const int rc = fb_run(fb, in, out, npart, chan_stride);
  (void)fb_plan_ready(fb, fold);
  const int rc2 = fold_part_plan_submitted(fold, slot);
  return rc != DSPSR_AMD_OK ? rc : rc2;
}

// perform_fold of a square-law state (dspsr -d 1, -d 2): the profile is npol 1 x ndim 1 (Intensity; PP of an object of one
// polarisation) or npol 2 x ndim 1 (PPQQ).  Fused where fold_is_fused_state says 1 or 2, the call does not take the two-pass path
// (k_rows_inv has no such epilogue) and no run reaches FOLD_FUSED_MAX_RUN; else Detection (fb_detect_square_law, on the
// object's own rows) and Fold.  The accumulators are scalars: no condition on a bound profile's address or span.
static int fb_perform_fold_sq(dspsr_amd_filterbank* fb, const float* in_f32_dev, uint64_t in_chan_stride, uint64_t in_pol_stride,
                              uint64_t in_step, const int8_t* raw_dev, int raw_layout, float scale, int state, dspsr_amd_fold* fold,
                              uint64_t npart)
{
  const char* fn = "dspsr_amd_filterbank_perform_fold";
  dspsr_amd_ctx* ctx = fb->ctx;
  const uint32_t npo = state == DSPSR_AMD_PPQQ ? 2u : 1u, nchan = fb->cfg.input_nchan * fb_out_C(fb);
  const char* sname = state == DSPSR_AMD_PPQQ ? "PPQQ" : fb->cfg.npol == 1 ? "PP" : "Intensity";
  if (state == DSPSR_AMD_PPQQ && fb->cfg.npol != 2)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "%s: PPQQ needs two polarisations (npol=%u)", fn, fb->cfg.npol);
  if (!fold->profile || fold->nchan != nchan || fold->npol != npo || fold->ndim != 1)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "%s: state=%d (%s) folds into a profile of nchan=%u npol=%u ndim=1 (is %u/%u/%u)", fn, state, sname,
                   nchan, npo, fold->nchan, fold->npol, fold->ndim);
  if (fold->folding_nbin != fold->nbin)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dsp::Fold::fold folding_nbin != output->nbin (%u != %u)", fold->folding_nbin, fold->nbin);
  if (npart > 0xffffffffull) return DSPSR_AMD_EINVAL;
  FbIn in;
  int rc = fb_input(fb, fn, in_f32_dev, in_pol_stride, in_step, raw_dev, raw_layout, scale, &in);
  if (rc != DSPSR_AMD_OK) return rc;
  const int fmode = dspsr_amd_filterbank_fold_is_fused_state(fb, state);
  FbOut probe = {};
  probe.kind = FB_OUT_FOLD;
  if ((fmode != 1 && fmode != 2) || fb_takes_two_pass(fb, in, probe) || fold_plan_max_run(fold) >= FOLD_FUSED_MAX_RUN) {
    const uint64_t ndat = npart * fb_out_nkeep(fb);
    if (!ndat) return DSPSR_AMD_OK;
    float* det = nullptr;
    rc = fb_detect_square_law(fb, fn, in, in_chan_stride, state, &det, 0, 0, npart);
    if (rc != DSPSR_AMD_OK) return rc;
    return dspsr_amd_fold_fold(fold, det, npo * fb_sq_own_row(ndat), fb_sq_own_row(ndat));
  }
  const uint32_t* d_start = nullptr;
  const Interval* d_iv = nullptr;
  PlanSlot* slot = nullptr;
  rc = fold_build_part_plan(fold, fb->g.nkeep, (uint32_t)npart, &d_start, &d_iv, &slot);
  if (rc != DSPSR_AMD_OK) return rc;
  return fb_run_with_plan(fb, fold, slot, in, fb_out_fold_sq(fold, state, npo, d_start, d_iv, (uint32_t)npart), npart, in_chan_stride);
}

extern "C" int dspsr_amd_filterbank_perform_fold(dspsr_amd_filterbank* fb, const float* in_f32_dev,
                                                 uint64_t in_chan_stride, uint64_t in_pol_stride, uint64_t in_step,
                                                 const int8_t* raw_dev, int raw_layout, float scale, int state,
                                                 dspsr_amd_fold* fold, uint64_t npart)
{
  if (!fb || !fold || (!in_f32_dev == !raw_dev)) return DSPSR_AMD_EINVAL;
  dspsr_amd_ctx* ctx = fb->ctx;
  if (fb_state_square_law(state))
    return fb_perform_fold_sq(fb, in_f32_dev, in_chan_stride, in_pol_stride, in_step, raw_dev, raw_layout, scale, state, fold, npart);
  if (fb->cfg.npol != 2)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_fold: Cannot detect polarization when npol != 2");
  if (state != DSPSR_AMD_COHERENCE && state != DSPSR_AMD_STOKES)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dspsr_amd_filterbank_perform_fold: invalid state=%d", state);
  const uint32_t nchan = fb->cfg.input_nchan * fb_out_C(fb);
  // profile shapes: npol 1 x ndim 4 (one float4 per bin, the CPU default, LoadToFoldConfig.C:104) or npol 2 x ndim 2 (rows
  // (PP, QQ) and (Re, Im): what the reference's GPU pipeline detects and folds, LoadToFold1.C:1105-1109)
  const bool planes2 = fold->npol == 2 && fold->ndim == 2;
  if (!fold->profile || fold->nchan != nchan || !((fold->npol == 1 && fold->ndim == 4) || planes2))
    return fb_fail(ctx, DSPSR_AMD_EINVAL,
                   "dspsr_amd_filterbank_perform_fold: fold shape must be nchan=%u with npol=1 ndim=4 or npol=2 ndim=2 (is %u/%u/%u)",
                   nchan, fold->nchan, fold->npol, fold->ndim);
  if (fold->folding_nbin != fold->nbin)
    return fb_fail(ctx, DSPSR_AMD_EINVAL, "dsp::Fold::fold folding_nbin != output->nbin (%u != %u)",
                   fold->folding_nbin, fold->nbin);
  if (npart > 0xffffffffull) return DSPSR_AMD_EINVAL;
  FbIn in;
  int rc = fb_input(fb, "dspsr_amd_filterbank_perform_fold", in_f32_dev, in_pol_stride, in_step, raw_dev, raw_layout, scale, &in);
  if (rc != DSPSR_AMD_OK) return rc;
  // In the fused kernel one workgroup owns a tile of channels for all parts of a launch (that keeps the sums in
  // time order), so it only pays when the channel tiles alone fill the chip: measured on MI355X, 512 tiles
  // (-F 1024:D -x 4096) +14 %, 128 tiles (-F 256:D) -13 %, 32 tiles (-F 512:D on a 50 MHz sub-band) 4x slower.
  // Below the threshold, and for the four-pass geometry, Detection and Fold run as separate launches on an
  // internal block -- the sums are bit-identical either way.
  // (a bound profile whose rows are not float4 aligned also takes the separate launches: the fold kernel adds scalars)
  const bool prof_vec4 = planes2 ? (fold->span % 2 == 0 && ((uintptr_t)fold->profile % 16) == 0)
                                 : (fold->span % 4 == 0 && ((uintptr_t)fold->profile % 16) == 0);
  if (dspsr_amd_filterbank_fold_is_fused(fb) == 3 && !planes2 && prof_vec4 && npart &&
      fold_plan_max_run(fold) >= FOLD_LONG_RUN && npart * (uint64_t)fb->g.nkeep < (1ull << 32)) {
    // Four-pass geometry (dsp::Convolution shapes, -F N:D with a long response) and wide phase bins: the second inverse pass
    // reduces its tile to the sums of the Tt-sample segments it holds and a second kernel adds those in time order -- the
    // detected time series (16 bytes per sample, written and read once) never reaches HBM.  Plans that do not qualify
    // (gaps from zero weights, short inner intervals, a fold that does not cover the call) take Detection + Fold below.
    bool ok = false;
    const uint32_t* d_off = nullptr; const uint32_t* d_blk = nullptr; const uint32_t* d_bs = nullptr;
    const Interval* d_siv = nullptr;
    PlanSlot* sslot = nullptr;
    rc = fold_build_segment_plan(fold, npart * (uint64_t)fb->g.nkeep, 1u << fb->g.logTt, &ok, &d_off, &d_blk, &d_bs, &d_siv, &sslot);
    if (rc != DSPSR_AMD_OK) return rc;
    if (ok) {
      const size_t need = ((size_t)fb->g.C * npart << (fb->g.logMf - fb->g.logTt)) * 8;       // segments x 2 pieces x float4
      if (!grow_device_buffer(ctx->stream, fb->msum, fb->msum_floats, need))
        return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform_fold: hipMalloc of %zu segment-sum bytes failed", need * sizeof(float));
      const FbOut sout = fb_out_segsum(fb->msum, fold, state, d_off, d_siv, d_blk, d_bs, (uint32_t)npart);
      return fb_run_with_plan(fb, fold, sslot, in, sout, npart, in_chan_stride);
    }
  }
  const int fmode = dspsr_amd_filterbank_fold_is_fused(fb);
  if ((fmode != 1 && fmode != 2) || !prof_vec4 || fold_plan_max_run(fold) >= FOLD_FUSED_MAX_RUN) {
    const uint64_t row = npart * fb_out_nkeep(fb) * 4;                       // floats per channel
    const size_t need = (size_t)row * nchan;
    if (!need) return DSPSR_AMD_OK;
    if (!grow_device_buffer(ctx->stream, fb->det, fb->det_floats, need))
      return fb_fail(ctx, DSPSR_AMD_ENOMEM, "dspsr_amd_filterbank_perform_fold: hipMalloc of %zu bytes failed", need * sizeof(float));
    // (ndim 2: the channel's two rows of npart*nkeep float2 one after the other)
    rc = fb_run(fb, in, fb_out_detected(fb->det, row, planes2 ? row / 2 : 0, state, planes2 ? 2u : 4u), npart, in_chan_stride);
    if (rc != DSPSR_AMD_OK) return rc;
    return dspsr_amd_fold_fold(fold, fb->det, row, planes2 ? row / 2 : 0);
  }
  const uint32_t* d_start = nullptr;
  const Interval* d_iv = nullptr;
  PlanSlot* slot = nullptr;
  rc = fold_build_part_plan(fold, fb->g.nkeep, (uint32_t)npart, &d_start, &d_iv, &slot);
  if (rc != DSPSR_AMD_OK) return rc;
  return fb_run_with_plan(fb, fold, slot, in, fb_out_fold(fold, state, planes2, d_start, d_iv, (uint32_t)npart), npart, in_chan_stride);
}

