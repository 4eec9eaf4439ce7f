"""dsp::SpectralKurtosis restated as loops (Signal/General/SpectralKurtosis.C, the CPU branch in FPT order), independent of the library:
float32 numpy scalars and arrays (one rounding per operation, x86 without fused multiply-add), sequential order, every counter.

    compute (:302-371), reset_mask / detect_tscr / detect_skfb / detect_fscr / count_zapped (:413-741), mask (:747-797).

The limits are arguments: the restatement does not know where they come from (tests/golden/sk_limits.json holds the reference's)."""
import numpy as np

F = np.float32
ZAP_ALL, ZAP_SKFB, ZAP_FSCR, ZAP_TSCR = 0, 1, 2, 3


def sums(rows, M, dtype=np.float32):
    """S1, S2 [npart][nchan][npol] of complex rows float32 [nchan][npol][2 * ndat], added sample by sample in `dtype`."""
    nchan, npol, nfloat = rows.shape
    npart = (nfloat // 2) // M
    x = rows[:, :, :2 * npart * M].astype(dtype).reshape(nchan, npol, npart, M, 2)
    sqld = x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]                    # :321: each product and the sum rounded on its own
    if npart == 0:
        z = np.zeros((0, nchan, npol), dtype)
        return z, z.copy()
    s1 = np.add.accumulate(sqld, axis=-1, dtype=dtype)[..., -1]             # sequential: S1_sum += sqld
    s2 = np.add.accumulate(sqld * sqld, axis=-1, dtype=dtype)[..., -1]
    return np.ascontiguousarray(s1.transpose(2, 0, 1)), np.ascontiguousarray(s2.transpose(2, 0, 1))


def estimate(s1, s2, m, m_fac):
    """M_fac * (M * (S2 / (S1*S1)) - 1), 0 where S1 == 0, in the dtype of the sums."""
    t = s1.dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        est = t(m_fac) * (t(m) * (s2 / (s1 * s1)) - t(1))
    return np.where(s1 == 0, t(0), est).astype(s1.dtype)


def compute(rows, M, no_tscr=False, dtype=np.float32):
    """-> estimates [npart][nchan][npol] (TFP), estimates_tscr [nchan][npol] (None when tscr is disabled or there is no part)."""
    s1, s2 = sums(rows, M, dtype)
    npart = s1.shape[0]
    est = estimate(s1, s2, M, (M + 1) // (M - 1))                           # :253: unsigned integer division
    if no_tscr or npart == 0:
        return est, None
    s1t = np.add.accumulate(s1, axis=0, dtype=dtype)[-1]                    # :329-330: += in part order
    s2t = np.add.accumulate(s2, axis=0, dtype=dtype)[-1]
    t = s1.dtype.type
    m_t = t(np.float32(M * npart))                                          # :354: float(M * npart)
    return est, estimate(s1t, s2t, m_t, (m_t + t(1)) / (m_t - t(1)))


class Detector:
    """The state SpectralKurtosis keeps over its calls: options, zap_counts[4], npart_total, the filtered / unfiltered sums and hits."""

    def __init__(self, nchan, npol, M, std_devs=3, chan_start=0, chan_end=0, no_fscr=False, no_tscr=False, no_ft=False):
        self.nchan, self.npol, self.M, self.std_devs = nchan, npol, M, std_devs
        self.chan_start, self.chan_end = chan_start, chan_end or nchan      # :419-420
        self.no_fscr, self.no_tscr, self.no_ft = no_fscr, no_tscr, no_ft
        self.zap_counts = np.zeros(4, np.uint64)
        self.npart_total = 0
        self.unfiltered_hits = 0
        self.filtered_hits = np.zeros(nchan, np.uint64)
        self.filtered_sum = np.zeros((nchan, npol), np.float32)
        self.unfiltered_sum = np.zeros((nchan, npol), np.float32)
        self.mask = None

    def reset_mask(self, npart):
        self.mask = np.zeros((npart, self.nchan), np.uint8)

    def detect_tscr(self, est_tscr, lower, upper):
        lower, upper = F(lower), F(upper)
        for ichan in range(self.chan_start, self.chan_end):
            zap = False
            for ipol in range(self.npol):
                V = est_tscr[ichan, ipol]
                if V > upper or V < lower:
                    zap = True
            if zap:
                self.mask[:, ichan] = 1
                self.zap_counts[ZAP_TSCR] += np.uint64(self.mask.shape[0])

    def detect_skfb(self, est, lower, upper):
        lower, upper = F(lower), F(upper)
        for ipart in range(est.shape[0]):
            for ichan in range(self.nchan):
                zap = False
                for ipol in range(self.npol):
                    V = est[ipart, ichan, ipol]
                    if V > upper or V < lower:
                        zap = True
                if zap:
                    self.mask[ipart, ichan] = 1
                    if self.chan_start < ichan < self.chan_end:             # :576, strict
                        self.zap_counts[ZAP_SKFB] += np.uint64(1)

    def detect_fscr(self, est):
        _M = F(self.M)
        mu2 = (F(4) * _M * _M) / ((_M - F(1)) * (_M + F(2)) * (_M + F(3)))  # :673
        nsig = F(1 + self.std_devs)
        for ipart in range(est.shape[0]):
            zap_ipart = False
            for ipol in range(self.npol):
                sk_avg, cnt = F(0), 0
                for ichan in range(self.chan_start, self.chan_end):
                    if self.mask[ipart, ichan] == 0:
                        sk_avg = F(sk_avg + est[ipart, ichan, ipol])
                        cnt += 1
                if cnt > 0:
                    sk_avg = F(sk_avg / F(cnt))
                    one_sigma = F(np.sqrt(F(mu2 / F(cnt))))
                    upper = F(F(1) + F(nsig * one_sigma))
                    lower = F(F(1) - F(nsig * one_sigma))
                    if sk_avg > upper or sk_avg < lower:
                        zap_ipart = True
            if zap_ipart:
                self.mask[ipart, :] = 1
                self.zap_counts[ZAP_FSCR] += np.uint64(self.nchan)

    def count_zapped(self, est):
        npart = est.shape[0]
        self.npart_total += npart * self.nchan                              # :434
        for ipart in range(npart):
            self.unfiltered_hits += 1
            for ichan in range(self.chan_start, self.chan_end):
                for ipol in range(self.npol):
                    self.unfiltered_sum[ichan, ipol] = F(self.unfiltered_sum[ichan, ipol] + est[ipart, ichan, ipol])
                if self.mask[ipart, ichan] == 1:
                    self.zap_counts[ZAP_ALL] += np.uint64(1)
                    continue
                for ipol in range(self.npol):
                    self.filtered_sum[ichan, ipol] = F(self.filtered_sum[ichan, ipol] + est[ipart, ichan, ipol])
                self.filtered_hits[ichan] += np.uint64(1)

    def detect(self, est, est_tscr, limits, limits_tscr):
        """SpectralKurtosis::detect (:413-454) on the estimates of one call; limits = (lower, upper).  Returns the mask."""
        self.reset_mask(est.shape[0])
        if est.shape[0] == 0:
            return self.mask
        if not self.no_tscr:
            self.detect_tscr(est_tscr, *limits_tscr)
        if not self.no_ft:
            self.detect_skfb(est, *limits)
        if not self.no_fscr:
            self.detect_fscr(est)
        self.count_zapped(est)
        return self.mask

    def statistics(self):
        return {"zap_counts": self.zap_counts.copy(), "npart_total": self.npart_total, "unfiltered_hits": self.unfiltered_hits,
                "filtered_hits": self.filtered_hits.copy(), "filtered_sum": self.filtered_sum.copy(),
                "unfiltered_sum": self.unfiltered_sum.copy()}


def mask_rows(rows, mask, M):
    """:773-796: the npart * M samples the mask covers, copied or zeroed; float32 [nchan][npol][2 * npart * M]."""
    nchan, npol, _ = rows.shape
    npart = mask.shape[0]
    out = rows[:, :, :2 * npart * M].copy()
    for ichan in range(nchan):
        for ipart in range(npart):
            if mask[ipart, ichan]:
                out[ichan, :, 2 * ipart * M:2 * (ipart + 1) * M] = 0
    return out


def same_statistics(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in
               ("zap_counts", "npart_total", "unfiltered_hits", "filtered_hits", "filtered_sum", "unfiltered_sum"))
