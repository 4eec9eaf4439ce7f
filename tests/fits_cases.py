"""dsp::FITSDigitizer with set_rescale_samples (Kernel/Formats/fits/FITSDigitizer.C), FPT branch, restated as loops: numpy scalars with
an explicit float32 / float64 at every step, sequential sums.  Written from the reference and independent of the kernels; it also
holds the case generators of tests/test_gpu_fits.py."""
import numpy as np

f32, f64 = np.float32, np.float64
INT_MIN = -2 ** 31


def digi_scales(nbit):
    """set_digi_scales (:14-45): (digi_mean, digi_scale, digi_min, digi_max), the first two as floats"""
    digi_sigma = f32(8)
    if nbit == 1:
        return f32(0.5), f32(1), 0, 1
    if nbit == 2:
        return f32(1.5), f32(1), 0, 3
    if nbit == 4:
        return f32(7.5), f32(7.5) / digi_sigma, 0, 15
    if nbit == 8:
        return f32(127.5), f32(127.5) / digi_sigma, 0, 255
    raise ValueError("dsp::FITSDigitizer::set_nbit nbit=%i not understood" % nbit)


def channel_map(nchan, flip_band, swap_band):
    """ChannelSort (:116-145) without sub-band swaps: input channel of every output channel"""
    half = nchan // 2
    out = []
    for k in range(nchan):
        ic = k
        if flip_band:
            ic = nchan - ic - 1
        if swap_band:
            ic = (ic + half) % nchan
        out.append(ic)
    return out


def to_int(d):
    """int(double) as the reference's x86 hosts convert (cvttsd2si): NaN and out-of-range values give INT_MIN"""
    d = f64(d)
    if d != d or d >= 2147483648.0 or d <= -2147483649.0:
        return INT_MIN
    return int(d)


def row_sums_sequential(x):
    """(:231-238) the sums of x and of the float product x*x, added in double in sample order"""
    s = q = f64(0.0)
    with np.errstate(over="ignore"):
        for v in x:
            v = f32(v)
            s = s + f64(v)
            q = q + f64(v * v)
    return s, q


def row_sums_cumsum(x):
    """row_sums_sequential without the Python loop: np.cumsum adds in element order, one double rounding per step (held to the loop
    in tests/test_fits_cases_host.py)"""
    x = np.asarray(x, f32)
    with np.errstate(over="ignore"):
        return np.cumsum(x.astype(f64))[-1], np.cumsum((x * x).astype(f64))[-1]


def row_sums_pairwise(x):
    """the same two sums in another order (np.sum adds pairwise): the only freedom the device has"""
    x = np.asarray(x, f32)
    return np.sum(x.astype(f64)), np.sum((x * x).astype(f64))


class FITSDigitizer:
    """One digitiser: pack(block [nchan][npol][nsblk] float32) -> (bytes, dat_scl, dat_offs)."""

    def __init__(self, nchan, npol, nbit, nsblk, nblock=1, constant=False, flip_band=False, swap_band=False, row_sums=row_sums_sequential):
        self.nchan, self.npol, self.nbit, self.nsblk, self.nblock, self.constant = nchan, npol, nbit, nsblk, nblock, constant
        self.map = channel_map(nchan, flip_band, swap_band)
        self.row_sums = row_sums
        self.digi_mean, self.digi_scale, self.digi_min, self.digi_max = digi_scales(nbit)
        stride = nchan * npol
        self.freq_total = np.zeros((nblock, stride), f64)
        self.freq_totalsq = np.zeros((nblock, stride), f64)
        self.scale = np.zeros(stride, f64)
        self.offset = np.zeros(stride, f64)
        self.rescale_idx = self.rescale_counter = 0
        self.regimes = []                       # what measure_scale did, call by call

    def measure_scale(self, block):             # :178-321
        if self.constant and self.rescale_counter > 0:
            self.regimes.append("constant")
            return
        nchan, npol, stride, n = self.nchan, self.npol, self.nchan * self.npol, self.nsblk
        if self.rescale_idx == self.nblock:
            self.rescale_idx = 0
        ft, fts = self.freq_total[self.rescale_idx], self.freq_totalsq[self.rescale_idx]
        ft[:] = 0.0
        fts[:] = 0.0
        idx = 0
        for ipol in range(npol):
            for ichan in range(nchan):
                s, q = self.row_sums(block[ichan, ipol, :n])
                ft[idx] += s
                fts[idx] += q
                idx += 1
        offset, scale = self.offset, self.scale
        with np.errstate(invalid="ignore"):
            if self.nblock == 1:
                self.regimes.append("single")
                self.rescale_counter = 1
                recip = f64(1.) / f64(n)
                for i in range(stride):
                    offset[i] = ft[i] * recip
                    scale[i] = np.sqrt(fts[i] * recip - offset[i] * offset[i])
                return
            if self.rescale_counter < self.nblock:
                self.regimes.append("filling")
                self.rescale_counter += 1
                offset[:] = 0.0
                scale[:] = 0.0
                for r in range(self.rescale_counter):
                    for j in range(stride):
                        offset[j] += self.freq_total[r, j]
                        scale[j] += self.freq_totalsq[r, j]
                recip = (f64(1.) / f64(n)) * (f64(1.) / f64(self.rescale_counter))
                for i in range(stride):
                    offset[i] = offset[i] * recip
                    scale[i] = np.sqrt(scale[i] * recip - offset[i] * offset[i])
                self.rescale_idx += 1
                return
            self.regimes.append("full")
            old_idx = self.rescale_idx + 1
            if old_idx == self.nblock:
                old_idx = 0
            recip = (f64(1.) / f64(n)) * (f64(1.) / f64(self.nblock))
            old_ft, old_fts = self.freq_total[old_idx], self.freq_totalsq[old_idx]
            for i in range(stride):
                old_offset = offset[i]
                offset[i] = offset[i] + (ft[i] - old_ft[i]) * recip
                scale[i] = np.sqrt(scale[i] * scale[i] - offset[i] * offset[i] + old_offset * old_offset + (fts[i] - old_fts[i]) * recip)
            self.rescale_idx += 1

    def levels(self, block):
        """rescale_pack's loop (:612-632): int levels [nsblk][npol][nchan] (TPF, output channel order)"""
        nchan, npol, n = self.nchan, self.npol, self.nsblk
        out = np.zeros((n, npol, nchan), np.int64)
        half = f64(0.5)
        with np.errstate(all="ignore"):
            for ichan in range(nchan):
                mapped = self.map[ichan]
                for ipol in range(npol):
                    m_scale = f32(f64(1.) / self.scale[ipol * nchan + mapped])
                    m_offset = f32(self.offset[ipol * nchan + mapped])
                    row = block[mapped, ipol]
                    for idat in range(n):
                        tmp = f32(f32(f32(row[idat]) - m_offset) * m_scale)
                        result = to_int(f64(f32(f32(tmp * self.digi_scale) + self.digi_mean)) + half)
                        out[idat, ipol, ichan] = max(min(result, self.digi_max), self.digi_min)
        return out

    def get_scales(self):                       # :675-699
        nchan, npol = self.nchan, self.npol
        dat_scl, dat_offs = np.zeros(nchan * npol, f32), np.zeros(nchan * npol, f32)
        with np.errstate(all="ignore"):
            for ichan in range(nchan):
                c = self.map[ichan]
                for ipol in range(npol):
                    dat_scl[ipol * nchan + ichan] = f32(self.scale[ipol * nchan + c] / f64(self.digi_scale))
                    dat_offs[ipol * nchan + ichan] = f32(self.offset[ipol * nchan + c])
        return dat_scl, dat_offs

    def pack(self, block):
        block = np.asarray(block, f32)
        assert block.shape == (self.nchan, self.npol, self.nsblk)
        self.measure_scale(block)
        lev = self.levels(block)
        scl, offs = self.get_scales()
        return pack_levels(lev.reshape(-1), self.nbit), scl, offs


def pack_levels(lev, nbit):
    """:639-656: sample isamp goes to byte isamp / spb, shifted by (spb - isamp % spb - 1) * nbit (most significant bits first)"""
    spb = 8 // nbit
    out = np.zeros(len(lev) // spb, np.uint8)
    for isamp, v in enumerate(lev):
        out[isamp // spb] += np.uint8((int(v) << ((spb - isamp % spb - 1) * nbit)) & 0xff)
    return out


def unpack_levels(b, nbit):
    """the levels of packed bytes, in sample order"""
    b = np.asarray(b, np.uint8).reshape(-1)
    spb = 8 // nbit
    shifts = (spb - 1 - np.arange(spb)) * nbit
    return ((b[:, None].astype(np.int64) >> shifts) & ((1 << nbit) - 1)).reshape(-1)


def fast_pack(dig, block):
    """What FITSDigitizer.pack computes, with the sample loop of `levels` vectorised (the same float32 / float64 operations element
    by element; tests/test_fits_cases_host.py holds it to the loop).  For the blocks of thousands of samples the GPU tests use."""
    block = np.asarray(block, f32)
    dig.measure_scale(block)
    nchan, npol = dig.nchan, dig.npol
    with np.errstate(all="ignore"):
        idx = np.array([[ipol * nchan + dig.map[k] for k in range(nchan)] for ipol in range(npol)])      # [npol][nchan out]
        m_scale = (f64(1.) / dig.scale[idx]).astype(f32)
        m_offset = dig.offset[idx].astype(f32)
        x = block[dig.map].transpose(2, 1, 0)                                                            # [n][npol][nchan out]
        tmp = (x - m_offset[None]) * m_scale[None]
        assert tmp.dtype == f32
        d = ((tmp * dig.digi_scale + dig.digi_mean).astype(f32)).astype(f64) + f64(0.5)
        bad = (d != d) | (d >= 2147483648.0) | (d <= -2147483649.0)
        lev = np.where(bad, f64(INT_MIN), np.trunc(d)).astype(np.int64)
    lev = np.clip(lev, dig.digi_min, dig.digi_max)
    spb = 8 // dig.nbit
    flat = lev.reshape(-1, spb)
    shifts = (spb - 1 - np.arange(spb)) * dig.nbit
    scl, offs = dig.get_scales()
    return (flat << shifts).sum(axis=1).astype(np.uint8), scl, offs


# ---- case generators --------------------------------------------------------------------------------------------------------------
EXACT_MAX = 2 ** 11
NSBLK_MAX = 2048            # the largest nsblk of the GPU tests


def exact_block(rng, nchan, npol, nsblk):
    """Integer-valued floats, |x| <= 2^11, a different mean and spread in every row: the sums of x (<= 2^11 * nsblk) and of x*x
    (<= 2^22 * nsblk) are integers below 2^53 for any nsblk <= 2^31, so they are exact in double IN ANY ORDER -- offsets, scales,
    floats and bytes of the reference do not depend on how its sums are taken, and the device must give its bits."""
    assert nsblk * EXACT_MAX ** 2 < 2 ** 53, "sums not exact in double"
    mean = rng.integers(-1200, 1200, (nchan, npol, 1))
    spread = rng.integers(1, 400, (nchan, npol, 1))
    x = np.clip(np.rint(mean + spread * rng.standard_normal((nchan, npol, nsblk))), -EXACT_MAX, EXACT_MAX)
    return x.astype(f32)


def noise_block(rng, nchan, npol, nsblk):
    """Gaussian noise with mean = 10 sigma, another sigma in every row"""
    sigma = rng.uniform(0.5, 40.0, (nchan, npol, 1))
    return (sigma * (10.0 + rng.standard_normal((nchan, npol, nsblk)))).astype(f32)


def ring_calls(nblock):
    """how many consecutive blocks visit every regime and wrap the ring twice"""
    return 2 * nblock + 3


NOISE_SEED = 20151124
NOISE_SHAPE = (24, 2, 2048)                     # nchan, npol, nsblk of the noise case
LEVEL_FRACTION = 1e-5                           # of the samples of a block may differ, each by one level
