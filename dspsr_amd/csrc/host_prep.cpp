// Host-side preparation that the reference also performs on the host:
//   dsp::Dedispersion   Signal/General/Dedispersion.C:216-248 (prepare), :291-331 (build),
//                       :383-475 (smearing), :478-556 (phases)
//   dsp::Response       Signal/General/Response.C:132-181 (match ordering), :259-344 (ndat rules),
//                       :649-700 (doswap);  dsp::Shape::rotate  Shape.C:222-266
//   optimal_fft_length  Signal/General/optimize_fft.c:63-127
//   BitTable scale      Kernel/Classes/BitTable.C:165-218
//   Fold bin plan       Signal/Pulsar/Fold.C:744-787
// The kernel is built in double, phases are rounded to float exactly where the reference rounds
// them (vector<float> phases), so the device receives the same numbers the CUDA engine would.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <complex>
#include <vector>

#include "../../include/dspsr_amd.h"

namespace {

const double dm_dispersion = 2.41e-4;                      // Dedispersion.C:28
const double smearing_buffer = 0.1;                        // Dedispersion.C:30
const unsigned smearing_samples_threshold = 16 * 1024 * 1024;   // Dedispersion.C:214

struct Dedisp {
  double centre_frequency, bandwidth, dm;
  unsigned nchan;
  std::vector<bool> supported;

  double delay_time(double f1, double f2) const            // :348-356
  {
    const double dispersion = dm / dm_dispersion;
    return dispersion * (1.0 / (f1 * f1) - 1.0 / (f2 * f2));
  }
  double smearing_time(int half) const                     // :383-430
  {
    const double abs_bw = fabs(bandwidth);
    double ch_abs_bw = abs_bw / double(nchan);
    double lower_ch_cfreq = centre_frequency - (abs_bw - ch_abs_bw) / 2.0;
    unsigned ichan = 0;
    while (ichan < supported.size() && !supported[ichan]) { lower_ch_cfreq += ch_abs_bw; ichan++; }
    if (half) { ch_abs_bw /= 2.0; lower_ch_cfreq += double(half) * ch_abs_bw; }
    return delay_time(lower_ch_cfreq - fabs(0.5 * ch_abs_bw), lower_ch_cfreq + fabs(0.5 * ch_abs_bw));
  }
  unsigned smearing_samples(int half) const                // :432-475
  {
    double tsmear = smearing_time(half);
    const double sampling_rate = fabs(bandwidth) / double(nchan) * 1e6;
    tsmear *= (1.0 + smearing_buffer);
    return unsigned(ceil(tsmear * sampling_rate));
  }
};

unsigned minimum_ndat(unsigned pos, unsigned neg)          // Response.C:259-275
{
  const double impulse_tot = pos + neg;
  if (impulse_tot == 0) return 0;
  unsigned min = unsigned(pow(2.0, ceil(log(impulse_tot) / log(2.0))));
  while (min <= impulse_tot) min *= 2;
  return min;
}

void swap_halves(std::complex<float>* buf, uint64_t npts, unsigned divisions)   // Response.C:649-700
{
  const uint64_t half = npts / (2 * divisions);
  for (unsigned d = 0; d < divisions; d++) {
    std::complex<float>* p1 = buf + 2 * half * d;
    std::swap_ranges(p1, p1 + half, p1 + half);
  }
}

bool get_dual_sideband(const dspsr_amd_dedispersion_config* c)   // Observation.C:80-87
{
  if (c->dual_sideband != -1) return c->dual_sideband == 1;
  return c->ndim == 2;
}

int fail(char* errbuf, size_t errlen, const char* fmt, unsigned a, unsigned b)
{
  if (errbuf && errlen) snprintf(errbuf, errlen, fmt, a, b);
  return DSPSR_AMD_EINVAL;
}

}  // namespace

extern "C" uint64_t dspsr_amd_optimal_fft_length(uint64_t nbadperfft, uint64_t nfft_max)   // optimize_fft.c:63-127
{
  if (!nbadperfft) return (uint64_t)-1;
  uint64_t nfft_min = (uint64_t)pow(2.0, ceil(log((double)nbadperfft) / log(2.0)));
  if (nfft_max && nfft_max < nfft_min) return (uint64_t)-1;
  uint64_t nfft = nfft_min;
  double timescale = ((double)nfft * log((double)nfft)) / (double)(nfft - nbadperfft);
  while (nfft_max == 0 || nfft * 2 < nfft_max) {
    const double prev = timescale;
    nfft *= 2;
    timescale = ((double)nfft * log((double)nfft)) / (double)(nfft - nbadperfft);
    if (timescale > prev) { nfft /= 2; break; }
  }
  return nfft;
}

extern "C" int dspsr_amd_dedispersion_prepare(const dspsr_amd_dedispersion_config* cfg,
                                              dspsr_amd_dedispersion_info* info, char* errbuf, size_t errlen)
{
  if (!cfg || !info || !cfg->nchan || cfg->bandwidth == 0.0) return DSPSR_AMD_EINVAL;
  Dedisp d;
  d.centre_frequency = cfg->centre_frequency;
  d.bandwidth = cfg->bandwidth;
  d.dm = cfg->dispersion_measure;
  d.nchan = cfg->nchan;
  d.supported.assign(cfg->nchan, true);
  const unsigned threshold = smearing_samples_threshold / cfg->nchan;        // Dedispersion.C:216-240
  unsigned ichan = 0, neg;
  while ((neg = d.smearing_samples(-1)) > threshold) {
    d.supported[ichan] = false;
    ichan++;
    if (ichan == cfg->nchan)
      return fail(errbuf, errlen, "dsp::Dedispersion::prepare smearing samples=%u exceeds threshold=%u", neg, threshold);
  }
  info->impulse_neg = neg;
  info->impulse_pos = d.smearing_samples(1);
  info->minimum_ndat = minimum_ndat(info->impulse_pos, info->impulse_neg);
  if (cfg->freq_res) {                                                          // Response::check_ndat :328-344
    if (cfg->ndat_max && cfg->freq_res > cfg->ndat_max)
      return fail(errbuf, errlen, "Response::check_ndat specified maximum ndat (%d) < specified ndat (%d)",
                  cfg->ndat_max, cfg->freq_res);
    if (cfg->freq_res < info->minimum_ndat)
      return fail(errbuf, errlen, "dsp::Response::check_ndat specified ndat (%d) < required minimum ndat (%d)",
                  cfg->freq_res, info->minimum_ndat);
    info->ndat = cfg->freq_res;
  } else {                                                                      // set_optimal_ndat :282-311
    if (cfg->ndat_max && cfg->ndat_max < info->minimum_ndat)
      return fail(errbuf, errlen,
                  "Response::set_optimal_ndat specified maximum ndat (%d) < required minimum ndat (%d)",
                  cfg->ndat_max, info->minimum_ndat);
    // (DM = 0: no smearing, nbadperfft == 0 -- optimal_fft_length fails and the reference throws, Response.C:300-305;
    //  an explicit resolution, -x, is the way through there as here)
    const uint64_t n = dspsr_amd_optimal_fft_length(info->impulse_pos + info->impulse_neg, cfg->ndat_max);
    if (n == (uint64_t)-1) return fail(errbuf, errlen, "Response::set_optimal_ndat optimal_fft_length failed%s", 0, 0);
    info->ndat = (uint32_t)n;
  }
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_dedispersion_build(const dspsr_amd_dedispersion_config* cfg, uint32_t ndat,
                                            float* kernel_host)
{
  if (!cfg || !kernel_host || !ndat || !cfg->nchan || cfg->bandwidth == 0.0) return DSPSR_AMD_EINVAL;
  const unsigned nchan = cfg->nchan;
  std::complex<float>* phasors = reinterpret_cast<std::complex<float>*>(kernel_host);

  // Dedispersion::build(vector<float>&, ndat, nchan)  :478-556  (Doppler_shift = 1)
  const double centrefreq = cfg->centre_frequency, bw = cfg->bandwidth;
  const double sign = bw / fabs(bw);
  const double chanwidth = bw / double(nchan);
  const double binwidth = chanwidth / double(ndat);
  double lower_cfreq = centrefreq - 0.5 * bw;
  if (!cfg->dc_centred) lower_cfreq += 0.5 * chanwidth;
  const double dispersion_per_MHz = 1e6 * cfg->dispersion_measure / dm_dispersion;
  const double highest_freq = centrefreq + 0.5 * fabs(bw - chanwidth);            // :504
  const double samp_int = 1.0 / chanwidth;                                         // :506 (microseconds, signed like bw)
  for (unsigned ichan = 0; ichan < nchan; ichan++) {
    const double chan_cfreq = lower_cfreq + double(ichan) * chanwidth;
    double delay = 0.0;
    if (cfg->fractional_delay) {                                                   // :524-533
      delay = dispersion_per_MHz * (1.0 / (chan_cfreq * chan_cfreq) - 1.0 / (highest_freq * highest_freq));
      delay = -fmod(delay, samp_int);
    }
    const double coeff = -sign * 2 * M_PI * dispersion_per_MHz / (chan_cfreq * chan_cfreq);
    const uint64_t spt = (uint64_t)ichan * ndat;
    for (unsigned ipt = 0; ipt < ndat; ipt++) {
      const double freq = double(ipt) * binwidth - 0.5 * chanwidth;
      const double delay_phase = -2.0 * M_PI * freq * delay;                       // :543
      const float phase = float(coeff * (freq * freq) / (chan_cfreq + freq) + delay_phase);   // stored as float :545
      phasors[spt + ipt] = std::polar(float(1.0), phase);                       // :320
    }
  }
  phasors[0] = 0;                                                                // :323

  // Response::match(const Observation*, unsigned)  Response.C:132-181
  const uint64_t npts = (uint64_t)nchan * ndat;
  if (cfg->input_nchan == 1) {
    if (get_dual_sideband(cfg)) swap_halves(phasors, npts, 1);
  } else {
    if (cfg->dc_centred) {
      // Dedispersion::prepare copied dc_centred from the input, so Response::dc_centred is already
      // true here and the half-channel rotate (Shape.C:222-266) is skipped -- same as the reference.
    }
    if (get_dual_sideband(cfg)) swap_halves(phasors, npts, cfg->input_nchan);
    if (cfg->swap) swap_halves(phasors, npts, 1);
  }
  phasors[0] = 0;                                                                // Dedispersion.C:278
  return DSPSR_AMD_OK;
}

// Dedispersion::SampleDelay::match (DedispersionSampleDelay.C:24-75) with Observation::get_centre_frequency(ichan)
// (Kernel/Classes/Observation.C:420-451)
extern "C" int dspsr_amd_dedispersion_sample_delays(double centre_frequency, double bandwidth, double dispersion_measure,
                                                    uint32_t nchan, double rate_hz, int swap, uint32_t nsub_swap,
                                                    int dc_centred, int64_t* delays_host)
{
  if (!delays_host || !nchan) return DSPSR_AMD_EINVAL;
  if (rate_hz == 0 || bandwidth == 0 || centre_frequency == 0) return DSPSR_AMD_EINVAL;   // :50-55 "invalid input"
  const double dispersion = dispersion_measure / 2.41e-4;                                 // dm_dispersion, Dedispersion.C:28
  const double base = dc_centred ? centre_frequency - 0.5 * bandwidth
                                 : centre_frequency - 0.5 * bandwidth + 0.5 * bandwidth / double(nchan);
  for (uint32_t ichan = 0; ichan < nchan; ichan++) {
    uint32_t c = ichan;
    if (swap) c = (c + nchan / 2) % nchan;
    if (nsub_swap) {
      const uint32_t sub_nchan = nchan / nsub_swap;
      c = (c / sub_nchan) * sub_nchan + (c % sub_nchan + sub_nchan / 2) % sub_nchan;
    }
    const double freq = base + double(c) * bandwidth / double(nchan);
    const double delay = dispersion * (1.0 / (centre_frequency * centre_frequency) - 1.0 / (freq * freq));
    delays_host[ichan] = int64_t(floor(delay * rate_hz + 0.5));
  }
  return DSPSR_AMD_OK;
}

extern "C" double dspsr_amd_eight_bit_scale(double input_spacing)               // BitTable.C:165-218
{
  const unsigned unique_values = 256;
  const double output_spacing = 1.0 / double(unique_values);
  const double output_middle = double(unique_values - 1) / 2.0;
  const unsigned input_middle = unique_values / 2;
  double cumulative_probability = 0.0, variance = 0.0;
  for (unsigned i = 0; i < unique_values; i++) {
    const double output = (double(i) - output_middle) * output_spacing;
    if (i < input_middle) {
      const double threshold = double(int(i + 1) - int(input_middle)) * input_spacing;
      const double cumulative = 0.5 * (1.0 + erf(threshold / sqrt(2.0)));   // NormalDistribution (ext)
      const double interval = cumulative - cumulative_probability;
      cumulative_probability = cumulative;
      variance += output * output * interval;
    }
  }
  variance *= 2.0;
  return (1.0 / sqrt(variance)) * output_spacing;
}

// One RUN of the plan loop of Fold.C:744-787 without walking its samples.
//   per sample:  if (!(phi >= 0 && phi < 1)) phi -= floor(phi);  ibin = unsigned(phi * nbin);  phi += phase_per_sample;
// The recurrence is a chain of rounded additions, so its values cannot be had by a multiplication -- but inside one binade
// [2^(e-1), 2^e) every phi is a multiple K u of the spacing u = 2^(e-53), and the rounded sum phi + pps is (K + round(pps / u)) u for
// every K as long as it stays in the binade and pps / u is not half-way between two integers: the chain is an exact arithmetic
// progression there, in integers.  The bin number is monotone along it, so the last sample of the run is found by bisection with the
// reference's own expression unsigned(phi * nbin).  A step that leaves the binade (or an undecided case: tie, phi tiny, pps < 0) is
// taken as the one rounded addition it is.  Same values as the sample-by-sample loop, bit for bit (tests/test_fold_plan_runs.py:
// against dspsr_amd_fold_binplan on random phases, steps and bin counts); cost per run instead of per sample -- at 50 MHz channel
// rates (`dspsr -F 8`) the loop was twice the time of the kernels of a block.
// In: *phi the state in front of the first sample (not normalised), nmax >= 1 samples available.  Out: the bin of the run, the
// number of its samples taken (<= nmax), *phi the state in front of the sample behind them.
namespace dspsr_amd {
static inline double pow2d(const int e)                      // 2^e for -1022 <= e <= 1023
{
  const uint64_t b = (uint64_t)(e + 1023) << 52;
  double d;
  memcpy(&d, &b, sizeof d);
  return d;
}
uint64_t fold_plan_run(double* phi_io, const double pps, const double double_nbin, const uint64_t nmax, uint32_t* ibin_out)
{
  double phi = *phi_io;
  if (!(phi >= 0.0 && phi < 1.0)) phi -= floor(phi);
  const uint32_t ibin = (uint32_t)(phi * double_nbin);
  *ibin_out = ibin;
  uint64_t n = 0;
  for (;;) {
    // sample n of the run has phase phi (in [0, 1), unless the input was not finite) and lies in bin ibin
    bool stepped = false;
    if (pps >= 0.0 && phi >= 0x1p-900 && phi < 1.0) {
      uint64_t bits;
      memcpy(&bits, &phi, sizeof bits);
      const int e = (int)((bits >> 52) & 0x7ff) - 1022;        // phi in [2^(e-1), 2^e) (normal: phi >= 2^-900), spacing u = 2^(e-53)
      const double r = pps * pow2d(53 - e);                    // pps / u: a power-of-two scaling, exact or inf (53 - e <= 953)
      if (r < 0x1p53) {
        const double fl = floor(r), frac = r - fl;
        if (frac != 0.5) {
          const uint64_t Ci = (uint64_t)(frac > 0.5 ? fl + 1.0 : fl);
          const uint64_t K = (bits & 0xfffffffffffffull) | (1ull << 52);      // phi / u: 2^52 <= K < 2^53
          const uint64_t kcap = Ci ? ((1ull << 53) - 1 - K) / Ci : ~0ull;      // phases (K + j Ci) u, j <= kcap, stay in the binade
          if (kcap > 0) {
            const double u = pow2d(e - 53);
            const uint64_t left = nmax - n - 1;                 // samples behind sample n that may still be taken
            const uint64_t jmax = kcap < left ? kcap : left;
            auto in_bin = [&](const uint64_t j) { return (uint32_t)(((double)(K + j * Ci) * u) * double_nbin) == ibin; };
            uint64_t j = jmax;                                  // last j <= jmax whose sample is in the bin (j = 0 is)
            if (!in_bin(jmax)) {
              // the bin number is monotone in j: bracket the last sample of the bin, starting from where the boundary
              // (ibin + 1) / nbin should be crossed, then bisect what is left (usually nothing)
              uint64_t lo = 0, hi = jmax;                       // in_bin(lo), !in_bin(hi)
              const double est = (((double)ibin + 1.0) / double_nbin - phi) / ((double)Ci * u);
              if (est >= 2.0 && est < (double)jmax) {
                const uint64_t g = (uint64_t)est;
                if (in_bin(g)) { lo = g; if (g + 2 < hi && !in_bin(g + 2)) hi = g + 2; }
                else { hi = g; if (g >= 2 && in_bin(g - 2)) lo = g - 2; }
              }
              while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (in_bin(mid)) lo = mid; else hi = mid;
              }
              j = lo;
            }
            n += j + 1;
            phi = j < kcap ? (double)(K + (j + 1) * Ci) * u : (double)(K + j * Ci) * u + pps;   // out of the binade: the rounded addition itself
            if (j < jmax || n == nmax) { *phi_io = phi; return n; }      // the next sample is in another bin, or none is left
            stepped = true;
          }
        }
      }
    }
    if (!stepped) {
      n++;
      phi += pps;
      if (n == nmax) { *phi_io = phi; return n; }
    }
    // the state in front of the next sample: is it still in the bin?
    if (!(phi >= 0.0 && phi < 1.0)) phi -= floor(phi);
    if ((uint32_t)(phi * double_nbin) != ibin) { *phi_io = phi; return n; }
  }
}
}  // namespace dspsr_amd

// the run list of the plan (test hook of fold_plan_run; dspsr_amd_fold_set_bins builds its plan with it): runs[i] = first sample,
// bin, samples; hits[nbin] +=
extern "C" int dspsr_amd_fold_binplan_runs(double phi, double phase_per_sample, uint32_t nbin, uint64_t ndat, uint64_t* run_offset,
                                           uint32_t* run_bin, uint64_t* run_hits, uint64_t cap, uint64_t* nruns, uint32_t* hits)
{
  if (!nbin || !nruns) return DSPSR_AMD_EINVAL;
  uint64_t nr = 0, idat = 0;
  uint32_t cur = nbin;
  while (idat < ndat) {
    uint32_t ibin;
    const uint64_t n = dspsr_amd::fold_plan_run(&phi, phase_per_sample, double(nbin), ndat - idat, &ibin);
    if (ibin >= nbin) return DSPSR_AMD_EINVAL;
    if (ibin != cur) {
      if (nr < cap) { run_offset[nr] = idat; run_bin[nr] = ibin; run_hits[nr] = 0; }
      nr++;
      cur = ibin;
    }
    if (nr - 1 < cap) run_hits[nr - 1] += n;
    if (hits) hits[ibin] += (uint32_t)n;
    idat += n;
  }
  *nruns = nr;
  return DSPSR_AMD_OK;
}

extern "C" int dspsr_amd_fold_binplan(double phi, double phase_per_sample, uint32_t nbin, uint64_t ndat,
                                      uint32_t* binplan, uint32_t* hits)         // Fold.C:744-787
{
  if (!nbin || (!binplan && ndat)) return DSPSR_AMD_EINVAL;
  const double double_nbin = double(nbin);
  for (uint64_t idat = 0; idat < ndat; idat++) {
    phi -= floor(phi);
    const unsigned ibin = unsigned(phi * double_nbin);
    phi += phase_per_sample;
    if (ibin >= nbin) return DSPSR_AMD_EINVAL;
    binplan[idat] = ibin;
    if (hits) hits[ibin]++;
  }
  return DSPSR_AMD_OK;
}

// ---- cyclic spectra: dsp::CyclicFold (Signal/Pulsar/CyclicFold.C) ---------------------------------------------------------
// The two bin plans of lag folding (CyclicFoldEngine::set_bin, CyclicFold.C:293-301, fed by the loop of Fold.C:744-787): the
// phase at the sample and half a sample later.  hits[] counts every sample (Fold.C:783).
extern "C" int dspsr_amd_cyclic_binplan(double phi, double phase_per_sample, uint32_t nbin, uint64_t ndat, uint32_t* plan0,
                                        uint32_t* plan1, uint32_t* hits)
{
  if (!nbin || ((!plan0 || !plan1) && ndat)) return DSPSR_AMD_EINVAL;
  const double double_nbin = double(nbin);
  const double bins_per_sample = phase_per_sample * double_nbin;
  for (uint64_t idat = 0; idat < ndat; idat++) {
    phi -= floor(phi);
    const double double_ibin = phi * double_nbin;
    const unsigned ibin = unsigned(double_ibin);
    phi += phase_per_sample;
    if (ibin >= nbin) return DSPSR_AMD_EINVAL;
    plan0[idat] = ibin;
    plan1[idat] = unsigned(double_ibin + 0.5 * bins_per_sample) % nbin;
    if (hits) hits[ibin]++;
  }
  return DSPSR_AMD_OK;
}

// CyclicFoldEngine::synch (CyclicFold.C:450-555): per (bin, pol, chan) the window of :519-537 when mover > 1, an unnormalised
// backward complex-to-real transform of nchan_spec = 2 nlag - 2 points (FTransform bcr1d: out[j] = sum over the Hermitian
// spectrum of z[k] e^{+2 pi i j k / n}; the imaginary parts of z[0] and z[n/2] do not enter), every mover-th point kept.
//   lags [bin][pol][chan][lag][re, im]  ->  out [chan * nchan_spec / mover + schan][pol][bin]
// The transform: the Hermitian extension through a radix-2 complex transform in float, twiddles rounded from double.
extern "C" int dspsr_amd_cyclic_lags_to_spectra(const float* lags, uint32_t nchan, uint32_t npol, uint32_t nbin, uint32_t nlag,
                                                uint32_t mover, float* out)
{
  if (!lags || !out || !nchan || !npol || !nbin || nlag < 2 || !mover) return DSPSR_AMD_EINVAL;
  const uint32_t n = 2 * nlag - 2;
  if ((n & (n - 1)) || n % mover) return DSPSR_AMD_EINVAL;
  const uint32_t nkeep = n / mover;
  uint32_t logn = 0;
  while ((1u << logn) < n) logn++;
  std::vector<std::complex<float>> tw(n / 2 ? n / 2 : 1), z(n);
  for (uint32_t k = 0; k < n / 2; k++)
    tw[k] = std::complex<float>((float)cos(2.0 * M_PI * k / n), (float)sin(2.0 * M_PI * k / n));
  std::vector<uint32_t> rev(n);
  for (uint32_t i = 0; i < n; i++) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < logn; b++) r |= ((i >> b) & 1u) << (logn - 1 - b);
    rev[i] = r;
  }
  std::vector<float> win(nlag, 1.0f);
  if (mover > 1)
    for (uint32_t ilag = 1; ilag < nlag; ilag++) {           // CyclicFold.C:523-532
      const float x = (M_PI / 3) * mover * ilag / ((float)(2 * nlag - 2));
      const float y = 0.5 * (1 + cos(2 * M_PI * float(ilag) / float(2 * nlag)));
      win[ilag] = y * sinf(x) / x;
    }
  for (uint32_t ibin = 0; ibin < nbin; ibin++)
    for (uint32_t ipol = 0; ipol < npol; ipol++)
      for (uint32_t ichan = 0; ichan < nchan; ichan++) {
        const float* l = lags + 2 * ((((size_t)ibin * npol + ipol) * nchan + ichan) * nlag);
        z[rev[0]] = std::complex<float>(l[0] * win[0], 0.f);
        for (uint32_t k = 1; k < nlag - 1; k++) {
          const std::complex<float> v(l[2 * k] * win[k], l[2 * k + 1] * win[k]);
          z[rev[k]] = v;
          z[rev[n - k]] = std::conj(v);
        }
        z[rev[nlag - 1]] = std::complex<float>(l[2 * (nlag - 1)] * win[nlag - 1], 0.f);
        for (uint32_t len = 2; len <= n; len <<= 1) {
          const uint32_t half = len / 2, step = n / len;
          for (uint32_t i = 0; i < n; i += len)
            for (uint32_t j = 0; j < half; j++) {
              const std::complex<float> w = tw[j * step], a = z[i + j], b = z[i + j + half];
              const std::complex<float> t(w.real() * b.real() - w.imag() * b.imag(), w.real() * b.imag() + w.imag() * b.real());
              z[i + j] = a + t;
              z[i + j + half] = a - t;
            }
        }
        for (uint32_t schan = 0; schan < nkeep; schan++)
          out[(((size_t)ichan * nkeep + schan) * npol + ipol) * nbin + ibin] = z[schan * mover].real();
      }
  return DSPSR_AMD_OK;
}

// ---- dspsr -R: dsp::RFIFilter (Signal/General/RFIFilter.C) on the host, as in the reference --------------------------------------
//
// fft::median_smooth is PSRCHIVE's and not part of the reference tree; restated: the window size is made odd, the result is
// computed from the unmodified data, the window at i is data[max(0, i - h) .. min(n - 1, i + h)] with h = wsize / 2, truncated at
// the edges, and the result is element len / 2 of the sorted window.
static void median_smooth(std::vector<float>& data, unsigned wsize)
{
  if (wsize % 2 == 0) wsize++;
  const long n = (long)data.size(), h = wsize / 2;
  const std::vector<float> in(data);
  std::vector<float> win;
  for (long i = 0; i < n; i++) {
    const long lo = std::max(0l, i - h), hi = std::min(n - 1, i + h);
    win.assign(in.begin() + lo, in.begin() + hi + 1);
    std::sort(win.begin(), win.end());
    data[i] = win[win.size() / 2];
  }
}

// RFIFilter::calculate (RFIFilter.C:105-162), operation by operation.  keep_zapped = 0 is the literal loop: a channel that does not
// trigger in a round gets 1 whatever happened to it before, and the loop ends only after a round without a trigger, so the mask
// it leaves is all ones and only the zeros in p0 / p1 survive.  keep_zapped = 1: a channel zapped in any round stays 0.
// cutoffs (may be NULL): the cutoff of each round, at most cutoff_cap stored -- what the reference prints as "round k cutoff = ...".
// A round whose triggers are all re-zaps (possible only with a cutoff below zero, where every zeroed channel triggers again and
// `variance -= 0` changes nothing) repeats for ever in the reference: DSPSR_AMD_ESTATE, the outputs as that round left them.
extern "C" int dspsr_amd_rfi_mask_calculate_log(float* p0ptr, float* p1ptr, uint32_t nchan_bp, uint32_t median_window,
                                                int keep_zapped, float* ptr, uint32_t* total_zapped_out, uint32_t* rounds_out,
                                                float* cutoffs, uint32_t cutoff_cap)
{
  if (!p0ptr || !p1ptr || !ptr || !nchan_bp || !median_window) return DSPSR_AMD_EINVAL;
  std::vector<float> spectrum(nchan_bp);
  unsigned ichan = 0;
  for (ichan = 0; ichan < nchan_bp; ichan++) spectrum[ichan] = p0ptr[ichan] + p1ptr[ichan];      // :116-117
  median_smooth(spectrum, median_window);                                                         // :119
  double variance = 0.0;
  for (ichan = 0; ichan < nchan_bp; ichan++) {                                                    // :122-128
    spectrum[ichan] -= (p0ptr[ichan] + p1ptr[ichan]);
    spectrum[ichan] *= spectrum[ichan];
    variance += spectrum[ichan];
  }
  variance /= nchan_bp;                                                                           // :130
  std::vector<char> ever(nchan_bp, 0);
  for (ichan = 0; ichan < nchan_bp; ichan++) ptr[ichan] = 1;
  bool zapped = true;
  unsigned round = 1, total_zapped = 0;
  int rc = DSPSR_AMD_OK;
  while (zapped) {                                                                                // :139-158
    const float cutoff = 16.0 * variance;
    if (cutoffs && round <= cutoff_cap) cutoffs[round - 1] = cutoff;
    zapped = false;
    round++;
    bool fresh = false;
    for (ichan = 0; ichan < nchan_bp; ichan++) {
      if (spectrum[ichan] > cutoff || (ichan && fabs(spectrum[ichan] - spectrum[ichan - 1]) > 2 * cutoff)) {
        variance -= spectrum[ichan] / nchan_bp;
        spectrum[ichan] = p0ptr[ichan] = p1ptr[ichan] = ptr[ichan] = 0.0;
        total_zapped++;
        zapped = true;
        if (!ever[ichan]) fresh = true;
        ever[ichan] = 1;
      } else if (!(keep_zapped && ever[ichan])) {
        ptr[ichan] = 1;
      }
    }
    if (zapped && !fresh) {
      rc = DSPSR_AMD_ESTATE;
      break;
    }
  }
  if (total_zapped_out) *total_zapped_out = total_zapped;
  if (rounds_out) *rounds_out = round - 1;
  return rc;
}

extern "C" int dspsr_amd_rfi_mask_calculate(float* p0, float* p1, uint32_t n, uint32_t median_window, int keep_zapped, float* mask,
                                            uint32_t* total_zapped, uint32_t* rounds)
{
  return dspsr_amd_rfi_mask_calculate_log(p0, p1, n, median_window, keep_zapped, mask, total_zapped, rounds, nullptr, 0);
}

// RFIFilter::match (const Response*) (RFIFilter.C:165-206), quirks included: expand = required / n in integers, elements past
// n * expand stay 1; with required < n the shrink loop runs `ip < expand` with expand == 0, so nothing is ever zapped and the
// result is all ones.  phasors: `required` complex floats with zero imaginary part.
extern "C" int dspsr_amd_rfi_mask_expand(const float* data, uint32_t ndat, uint64_t required, float* phasors)
{
  if (!data || !ndat || !phasors) return DSPSR_AMD_EINVAL;
  const uint64_t expand = required / ndat, shrink = required ? ndat / required : 0;
  for (uint64_t i = 0; i < required; i++) {
    phasors[2 * i] = 1.0f;
    phasors[2 * i + 1] = 0.0f;
  }
  if (expand) {
    for (uint64_t idat = 0; idat < ndat; idat++)
      for (uint64_t ip = 0; ip < expand; ip++) phasors[2 * (idat * expand + ip)] = data[idat];
  } else if (shrink) {
    for (uint64_t idat = 0; idat < required; idat++)
      for (uint64_t ip = 0; ip < expand; ip++)
        if (data[idat * shrink + ip] == 0.0) phasors[2 * idat] = 0.0f;
  }
  return DSPSR_AMD_OK;
}

// Response::operator *= (Response.C:73-104) through Response::operate (:429-441): kernel[i] = phasors[i] * kernel[i], complex.
// (One product or difference per statement: nothing here may be contracted into a fused multiply-add.)
extern "C" int dspsr_amd_response_multiply(float* kernel, const float* phasors, uint64_t ncomplex)
{
  if (!kernel || !phasors) return DSPSR_AMD_EINVAL;
  for (uint64_t i = 0; i < ncomplex; i++) {
    const float d_r = kernel[2 * i], d_i = kernel[2 * i + 1], f_r = phasors[2 * i], f_i = phasors[2 * i + 1];
    const float rr = f_r * d_r;
    const float ii = f_i * d_i;
    const float ir = f_i * d_r;
    const float ri = f_r * d_i;
    kernel[2 * i] = rr - ii;
    kernel[2 * i + 1] = ir + ri;
  }
  return DSPSR_AMD_OK;
}

// ---- spectral-kurtosis limits: dsp::SKLimits::calc_limits (Signal/Statistics/SKLimits.C:29-100) ----------------------------
// The SK estimator of M samples follows a Pearson type IV distribution (PearsonIV.C:28-83: moments, r, m, v, a, lamda and the
// log of its normalisation); the limits are where its cumulative and complementary cumulative functions equal the one-sided tail
// of a Gaussian at std_devs sigma, found by Newton's iteration on their logarithms.  Everything that decides convergence is kept:
// the integrals are Romberg's with a FLOAT precision of 1e-12 compared against a double, 18 refinements and an extrapolation over
// 5 points that starts one refinement late (Romberg.h:27-58), open (three-fold midpoint) after the change of variable 1/x for the
// tails and closed (trapezoid) between -1 / +1 and x; Neville's tableau runs n-2 columns (Neville.h:43); Newton is clamped to
// [1e-4, 10], stops at dx^2 <= (x * 1e-12)^2 and gives up after 100 steps (NewtonRaphson.h:36-54).  An integral or an iteration
// that gives up makes the reference fall back to the starting guess 1 -+ std_devs * sqrt(4 / M) (SKLimits.C:75-94).
namespace {

struct sk_failed {};                                        // the reference's Error thrown by Romberg or NewtonRaphson

struct pearson_iv {
  double m, v, a, lamda, logk;

  explicit pearson_iv(const unsigned sk_m)                  // PearsonIV::prepare
  {
    const double M = (double)sk_m;
    const double mu1 = 1;
    const double mu2 = (4 * M * M) / ((M - 1) * (M + 2) * (M + 3));
    double beta1 = (4 * (M + 2) * (M + 3) * (5 * M - 7) * (5 * M - 7));
    beta1 /= ((M - 1) * (M + 4) * (M + 4) * (M + 5) * (M + 5));
    double beta2 = 3 * (M + 2) * (M + 3) * (M * M * M + 98 * M * M - 185 * M + 78);
    beta2 /= ((M - 1) * (M + 4) * (M + 5) * (M + 6) * (M + 7));
    const double r = (6 * (beta2 - beta1 - 1)) / (2 * beta2 - 3 * beta1 - 6);
    m = (r + 2) / 2;
    v = -1 * (r * (r - 2) * sqrt(beta1));
    v /= sqrt(16 * (r - 1) - beta1 * (r - 2) * (r - 2));
    a = 0.25 * sqrt(mu2 * ((16 * (r - 1)) - (beta1 * (r - 2) * (r - 2))));
    lamda = mu1 - 0.25 * (r - 2) * sqrt(mu2) * sqrt(beta1);
    logk = log_normal();
  }

  double log_normal() const                                 // PearsonIV.C:117-139
  {
    double x = m;
    const double y = 0.5 * v;
    const double y2 = y * y;
    const double xmin = (2 * y2 > 10.0) ? 2 * y2 : 10.0;
    double logr = 0, s = 1, p = 1, f = 0;
    while (x < xmin) {
      const double t = y / x++;
      logr += log(1 + t * t);
    }
    while (p > s * 2.2204460492503131e-16) {                // DBL_EPSILON
      p *= y2 + f * f;
      p /= x++ * ++f;
      s += p;
    }
    return log(0.5 * M_2_SQRTPI / a) - (logr + log(s)) + lgamma(m) - lgamma(m - 0.5);
  }

  double density(const double x) const                      // PearsonIV::operator()
  {
    const double a1 = (x - lamda) / a;
    const double a2 = 1 + a1 * a1;
    const double a3 = v * atan(a1);
    return exp(logk - 1 * m * log(a2) - a3);
  }
};

// the integrands of PearsonIV::cf / ccf: the density, OneOver(density) and Minus(OneOver(density)) (Romberg.h:64-118)
enum sk_integrand { SK_PLAIN, SK_ONE_OVER, SK_MINUS_ONE_OVER };
static double sk_eval(const pearson_iv& p, const sk_integrand kind, const double arg)
{
  if (kind == SK_PLAIN) return p.density(arg);
  if (kind == SK_ONE_OVER) return -p.density(1.0 / arg) / (arg * arg);
  const double t = -arg;
  return -(-p.density(1.0 / t) / (t * t));
}

static void sk_neville(const double* xa, const double* ya, const unsigned n, const double x, double& y, double& dy)
{
  unsigned ns = 0;
  double c[8], d[8];
  double dif = fabs(x - xa[0]);
  for (unsigned i = 0; i < n; i++) {
    const double dift = fabs(x - xa[i]);
    if (dift < dif) {
      ns = i;
      dif = dift;
    }
    c[i] = ya[i];
    d[i] = ya[i];
  }
  y = ya[ns];
  ns--;
  dy = 0;
  for (unsigned m = 1; m < n - 1; m++) {                    // (n-2 columns, as the reference)
    for (unsigned i = 0; i < n - m; i++) {
      const double ho = xa[i] - x;
      const double hp = xa[i + m] - x;
      const double w = c[i + 1] - d[i];
      double den = ho - hp;
      den = w / den;
      d[i] = hp * den;
      c[i] = ho * den;
    }
    if (2 * ns >= (n - m)) {
      dy = d[ns];
      ns--;
    } else
      dy = c[ns + 1];
    y += dy;
  }
}

// Romberg<Trapezoid> (open == false) or Romberg<MidPoint> (open == true) of the integrand from x1 to x2
static double sk_romberg(const pearson_iv& p, const sk_integrand kind, const bool open, const double x1, const double x2)
{
  const unsigned extrapolate = 5, iterations = 18;
  const float precision = 1.0e-12;                          // a float, compared against a double below
  const double order_squared = open ? 9.0 : 4.0;
  double h[iterations + 1], s[iterations];
  double rule = 0;                                          // the refinement rule's running estimate (Trapezoid::s, MidPoint::s)
  h[0] = 1.0;
  double ss = 0, dss = 0;
  for (unsigned j = 0; j < iterations; j++) {
    if (j == 0) {
      rule = open ? (x2 - x1) * sk_eval(p, kind, 0.5 * (x1 + x2)) : 0.5 * (x2 - x1) * (sk_eval(p, kind, x1) + sk_eval(p, kind, x2));
    } else {
      unsigned it = 1;
      for (unsigned k = 1; k < j; k++) it *= open ? 3 : 2;
      const double tnm = it;
      double sum = 0.0;
      if (open) {                                           // MidPoint.h:34-47
        const double del = (x2 - x1) / (3.0 * tnm);
        const double ddel = del + del;
        double x = x1 + 0.5 * del;
        for (unsigned k = 0; k < it; k++) {
          sum += sk_eval(p, kind, x);
          x += ddel;
          sum += sk_eval(p, kind, x);
          x += del;
        }
        rule = (rule + (x2 - x1) * sum / tnm) / 3.0;
      } else {                                              // Trapezoid.h:34-44
        const double del = (x2 - x1) / tnm;
        double x = x1 + 0.5 * del;
        for (unsigned k = 0; k < it; k++) {
          sum += sk_eval(p, kind, x);
          x += del;
        }
        rule = 0.5 * (rule + (x2 - x1) * sum / tnm);
      }
    }
    s[j] = rule;
    if (j >= extrapolate) {
      sk_neville(h + j - extrapolate, s + j - extrapolate, extrapolate, 0.0, ss, dss);
      if (fabs(dss) <= precision) return ss;
    }
    h[j + 1] = h[j] / order_squared;
  }
  throw sk_failed();
}

static double sk_cf(const pearson_iv& p, const double x)    // PearsonIV::cf
{
  if (x < -1) return sk_romberg(p, SK_MINUS_ONE_OVER, true, 0., -1 / x);
  return sk_romberg(p, SK_MINUS_ONE_OVER, true, 0., 1.) + sk_romberg(p, SK_PLAIN, false, -1., x);
}

static double sk_ccf(const pearson_iv& p, const double x)   // PearsonIV::ccf
{
  if (x > 1) return sk_romberg(p, SK_ONE_OVER, true, 1 / x, 0.);
  return sk_romberg(p, SK_ONE_OVER, true, 1., 0.) + sk_romberg(p, SK_PLAIN, false, x, 1.);
}

// NewtonRaphson::operator() on log cf (upper == false) or log ccf (upper == true) with limits [1e-4, 10]
static double sk_newton(const pearson_iv& p, const bool upper, const double y, double guess_x)
{
  const double precision = 1e-12, lower_limit = 1e-4, upper_limit = 10;
  for (unsigned i = 0; i < 100; i++) {
    const double c = upper ? sk_ccf(p, guess_x) : sk_cf(p, guess_x);     // (log_cf and dlog_cf integrate the same thing twice)
    const double f = log(c);
    const double df = upper ? -1 * p.density(guess_x) / c : p.density(guess_x) / c;
    const double dx = (f - y) / df;
    guess_x -= dx;
    if (guess_x < lower_limit) guess_x = lower_limit;
    if (guess_x > upper_limit) guess_x = upper_limit;
    if (dx * dx <= (guess_x * precision) * (guess_x * precision)) return guess_x;
  }
  throw sk_failed();
}

}  // namespace

extern "C" int dspsr_amd_sk_limits(uint32_t M, uint32_t std_devs, float* lower, float* upper)
{
  if (!lower || !upper) return DSPSR_AMD_EINVAL;
  *lower = *upper = 0;
  if (M < 32 || std_devs == 0) return DSPSR_AMD_EINVAL;     // below M = 24 the Pearson IV parameters are not finite
  const double percent_std_devs = erf((float)std_devs / sqrt(2));
  const double target = (1 - percent_std_devs) / 2.0;
  const double one_std_dev = sqrt(4.0 / (double)M);
  const double factor = one_std_dev * std_devs;
  double lo, hi;
  if (M >= 32768) {                                         // SKLimits.C:46-51: the Gaussian limit
    lo = 1.0f - factor;
    hi = 1.0f + factor;
  } else {
    const pearson_iv p(M);
    lo = 1 - factor;
    try {
      lo = sk_newton(p, false, log(target), lo);
    } catch (const sk_failed&) {
    }
    hi = 1 + factor;
    try {
      hi = sk_newton(p, true, log(target), hi);
    } catch (const sk_failed&) {
    }
  }
  *lower = (float)lo;                                       // SpectralKurtosis.C:390-391
  *upper = (float)hi;
  return DSPSR_AMD_OK;
}
