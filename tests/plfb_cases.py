"""The cases of the phase-locked filterbank's device tests (tests/test_gpu_plfb.py), built without a device so that the host suite
can check what the bit-for-bit comparison rests on (tests/test_plfb_host.py)."""
import functools

import numpy as np

import plfb_reference as pr

SENTINEL_UNITS = 5            # the profile holds 5 nchan^2 everywhere before a call: an exact value like the sums

# (ndim, nchan, npol_in, npol_out, nchan_in, nbin, tone, rot, overlap): tone "dc" or "half" (the half-band tone: (-1)^n for
# Analytic rows, cos(pi n / 2) for Nyquist rows).  The windows per bin are 0, 1, Tp - 1, Tp, Tp + 1, 2 Tp + 1 (Tp = 8192 / nchan
# windows = a tile's 16384 / nchan columns of (window, polarisation)), bin b taking entry (b + rot) % 6, bins from 6 on none
# except the last; several tiles, hence several segments, and bins that span two of them.
EXACT = [
    (2, 2, 2, 4, 1, 64, "half", 0, False),
    (2, 16, 2, 1, 1, 1025, "dc", 0, False),
    (2, 32, 2, 2, 3, 3, "half", 3, False),
    (2, 256, 1, 1, 3, 64, "dc", 0, False),
    (2, 512, 2, 4, 3, 1025, "half", 0, False),
    (2, 4096, 2, 2, 1, 2, "dc", 2, False),
    (2, 8192, 2, 4, 3, 64, "half", 0, False),
    (2, 8192, 2, 1, 1, 3, "dc", 3, False),
    (2, 256, 2, 4, 1, 3, "half", 0, True),
    (1, 2, 2, 4, 1, 64, "half", 0, False),
    (1, 16, 2, 2, 3, 1025, "dc", 0, False),
    (1, 256, 1, 1, 3, 3, "half", 3, False),
    (1, 8192, 2, 4, 3, 2, "dc", 4, False),
    (1, 8192, 2, 1, 1, 64, "half", 0, False),
    (1, 16, 2, 4, 1, 2, "dc", 0, True),
]
IDS = ["ndim%d-nchan%d-pol%dto%d-chan%d-nbin%d-%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], "-overlap" if c[8] else "") for c in EXACT]


def _tone(kind, ndim, t):
    if kind == "dc":
        return np.ones(t.shape)
    return np.where(t % 2 == 0, 1.0, -1.0) if ndim == 2 else np.array([1.0, 0.0, -1.0, 0.0])[t % 4]


@functools.lru_cache(maxsize=None)
def exact_case(index):
    """rows (float64 [nchan_in][npol_in][ndat * ndim], NaN outside the windows), starts, bins, the float64 reference"""
    ndim, nchan, npol_in, npol_out, nchan_in, nbin, tone, rot, overlap = EXACT[index]
    rng = np.random.default_rng(100 + index)
    tp = 8192 // nchan
    ndat_fft = nchan * (2 if ndim == 1 else 1)
    if overlap:
        nwin = 40
        bins = (np.arange(nwin) * 2 + 1) % nbin
        step = max(ndat_fft // 3, 1)
        starts = np.arange(nwin) * step
        amp = np.repeat(rng.integers(1, 4, (nchan_in, npol_in, 1, 2)), nwin, axis=2)       # one amplitude for the whole row
    else:
        pattern = [0, 1, tp - 1, tp, tp + 1, 2 * tp + 1]
        counts = [pattern[(b + rot) % 6] if b < 6 else 0 for b in range(nbin)]
        if nbin > 6:
            counts[-1] = 2
        bins = rng.permutation(np.repeat(np.arange(nbin), counts))
        nwin = len(bins)
        starts = np.cumsum(ndat_fft + rng.integers(0, 4, nwin)) - ndat_fft                 # gaps of 0 .. 3 samples, odd starts too
        starts -= starts[0] - 1
        amp = rng.integers(-3, 4, (nchan_in, npol_in, nwin, 2))
        amp[..., 0] += (amp[..., 0] == 0) * 2
    ndat = int(starts[-1]) + ndat_fft                                                        # the last window ends on the last sample
    rows = np.full((nchan_in, npol_in, ndat, ndim), np.nan)
    t = starts[:, None] + np.arange(ndat_fft)[None, :]
    tv = _tone(tone, ndim, t)
    for c in range(nchan_in):
        for p in range(npol_in):
            if ndim == 2:
                rows[c, p, t, 0] = amp[c, p, :, 0, None] * tv
                rows[c, p, t, 1] = amp[c, p, :, 1, None] * tv
            else:
                rows[c, p, t, 0] = amp[c, p, :, 0, None] * tv
    rows = rows.reshape(nchan_in, npol_in, ndat * ndim)
    ref = pr.plfb_loop(rows, ndim, nchan, npol_out, nbin, starts, bins, np.float64)
    return rows, starts.astype(np.uint64), bins.astype(np.uint32), ref, ndat


NOISE = [(2, n) for n in (2, 16, 32, 256, 512, 4096, 8192)] + [(1, n) for n in (2, 16, 256, 8192)]


def noise_case(ndim, nchan, seed=7):
    """Gaussian rows [2][2][ndat * ndim], 50 overlapping windows over 5 bins; (rows float32, starts, bins, float64 reference,
    error figure of the float32 strict-order restatement)"""
    rng = np.random.default_rng(seed + nchan + ndim)
    ndat_fft = nchan * (2 if ndim == 1 else 1)
    nwin, nbin = 50, 5
    starts = np.arange(nwin, dtype=np.uint64) * np.uint64(ndat_fft // 2 + 1)
    bins = ((np.arange(nwin) * 3) % nbin).astype(np.uint32)
    ndat = int(starts[-1]) + ndat_fft
    rows = rng.standard_normal((2, 2, ndat * ndim)).astype(np.float32)
    ref = pr.plfb_loop(rows, ndim, nchan, 4, nbin, starts, bins, np.float64)
    f32 = pr.plfb_loop(rows, ndim, nchan, 4, nbin, starts, bins, np.float32)
    assert f32.dtype == np.float32
    e_f32 = np.abs(f32.astype(np.float64) - ref).max() / np.abs(ref).max()
    return rows, starts, bins, ref, ndat, e_f32
