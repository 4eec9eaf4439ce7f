"""Two-bit voltages: the loop restatements the two-bit tests compare against, and the generator of their streams.

  * unpack_restated: TwoBitFour::prepare / unpack (TwoBitFour.h:42-89) + ExcisionUnpacker::excision_unpack (excision_unpack.h:54-100)
    per digitiser, byte by byte with the two lookup tables the reference builds (nlow_lookup, the per-n_low value block);
  * mask_restated: WeightedTimeSeries::mask_weights as "a window is bad where any row is";
  * ja98_restated: Jenet & Anderson (1998) eq. 41 in float64 with its own inverse of erf (bisection), independent of dspsr_amd.twobit;
  * stream: a 2-bit stream per case -- Gaussian noise of a chosen sigma per window quantised at +-threshold into the chosen code,
    with chosen windows set to all-zero bytes, to sigma x 8 (too few low states), to sigma / 8 (too many), or to exactly nlow_min /
    nlow_max low states (kept, at the edge).

No device, no library: numpy only.
"""
import math

import numpy as np

OFFSET_BINARY, SIGN_MAGNITUDE, TWOS_COMPLEMENT = 0, 1, 2
TABLE_TYPES = (OFFSET_BINARY, SIGN_MAGNITUDE, TWOS_COMPLEMENT)
THRESHOLD = 0.9674


def unique_values(table_type, lo, hi):
    """TwoBitTable::generate_unique_values (TwoBitTable.C:42-70): the value of codes 0 ... 3."""
    lo, hi = np.float32(lo), np.float32(hi)
    return {OFFSET_BINARY: [-hi, -lo, lo, hi], SIGN_MAGNITUDE: [lo, hi, -lo, -hi], TWOS_COMPLEMENT: [lo, hi, -hi, -lo]}[table_type]


def code_of(table_type, negative, high):
    """The 2-bit code of a sample with that sign and magnitude (the inverse of unique_values)."""
    vals = unique_values(table_type, 1.0, 2.0)
    return vals.index(np.float32((-1.0 if negative else 1.0) * (2.0 if high else 1.0)))


def low_codes(table_type):
    vals = unique_values(table_type, 1.0, 2.0)
    return [c for c in range(4) if abs(vals[c]) == 1.0]


def byte_samples(byte):
    """The four codes of a byte, first sample in the two most significant bits (BitTable MostToLeast, BitTable.C:154-163)."""
    return [(byte >> 6) & 3, (byte >> 4) & 3, (byte >> 2) & 3, byte & 3]


def unpack_restated(block, table_type, npol, nsample, nlow_min, nlow_max, levels):
    """block: uint8, whole windows; byte k belongs to digitiser k % npol.  levels: float32 [nlow_max - nlow_min + 1][2].
    Returns (rows float32 [npol][nwindow * nsample], weights uint32 [npol][nwindow] before the mask, n_low uint32 the same shape)."""
    block = np.asarray(block, dtype=np.uint8).ravel()
    per = (nsample // 4) * npol
    assert nsample % 4 == 0 and block.size % per == 0
    nwindow = block.size // per
    lows = low_codes(table_type)
    nlow_lookup = [sum(1 for c in byte_samples(b) if c in lows) for b in range(256)]          # TwoBitFour::nlow_build
    rows = np.zeros((npol, nwindow * nsample), dtype=np.float32)
    weights = np.ones((npol, nwindow), dtype=np.uint32)                                      # neutral_weights
    n_lows = np.zeros((npol, nwindow), dtype=np.uint32)
    nbyte = nsample // 4
    for idig in range(npol):
        stream = block[idig::npol]                                                           # input offset idig, increment npol
        for wt in range(nwindow):
            window = stream[wt * nbyte:(wt + 1) * nbyte]
            nlow, total = 0, 0
            for b in window:                                                                 # prepare
                nlow += nlow_lookup[b]
                total += int(b)
            bad = total == 0
            n_low = nlow
            use = min(max(nlow, nlow_min), nlow_max)
            vals = unique_values(table_type, levels[use - nlow_min][0], levels[use - nlow_min][1])
            o = wt * nsample
            for b in window:                                                                 # unpack
                for c in byte_samples(int(b)):
                    rows[idig, o] = vals[c]
                    o += 1
            n_lows[idig, wt] = n_low
            if bad or n_low < nlow_min or n_low > nlow_max:
                weights[idig, wt] = 0
                rows[idig, wt * nsample:(wt + 1) * nsample] = 0.0
    return rows, weights, n_lows


def mask_restated(weights):
    w = np.array(weights, dtype=np.uint32)
    bad = (w == 0).any(axis=0)
    w[:, bad] = 0
    return w


def erf_inverse_bisect(p):
    lo, hi = 0.0, 6.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if math.erf(mid) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def ja98_restated(phi, threshold=THRESHOLD):
    """(lo, hi, sigma) of JA98 eq. 41 for a fraction phi of low states, float64."""
    x = erf_inverse_bisect(phi)
    sigma = threshold / (math.sqrt(2.0) * x)
    e = 2.0 * x / math.sqrt(math.pi) * math.exp(-x * x)
    return sigma * math.sqrt(1.0 - e / phi), sigma * math.sqrt(1.0 + e / (1.0 - phi)), sigma


def levels_restated(nsample, nlow_min, nlow_max, threshold=THRESHOLD):
    out = np.empty((nlow_max - nlow_min + 1, 2), dtype=np.float32)
    for k, nlo in enumerate(range(nlow_min, nlow_max + 1)):
        use = min(max(nlo, 1), nsample - 1)
        p_in = float(np.float32(use) / np.float32(nsample))
        out[k] = ja98_restated(p_in, threshold)[:2]
    return out


def limits_restated(nsample, threshold=THRESHOLD, cutoff=10.0):
    """ExcisionUnpacker::set_limits with float32 intermediates (written out once more, for the generator alone)."""
    f = np.float32
    if cutoff == 0:
        return 0, nsample
    m = math.erf(threshold / math.sqrt(2.0))
    mean, var = f(float(f(nsample)) * m), f(float(f(nsample)) * m * (1.0 - m))
    spread = f(f(cutoff) * f(np.sqrt(var)))
    nmax = min(int(f(mean + spread)), nsample - 1)
    nmin = 1 if float(spread) >= float(mean) + 1.0 else int(f(mean - spread))
    return nmin, nmax


# ---- the generator -------------------------------------------------------------------------------------------------------------
# what a window of a digitiser is made of
NOISE, ZERO, LOUD, QUIET, EXACT_MIN, EXACT_MAX = "noise", "zero", "loud", "quiet", "exact_min", "exact_max"
# nine windows per digitiser: every excision cause, both kept edges, a window bad in one polarisation and good in the other (3, 4)
KINDS = ((NOISE, ZERO, EXACT_MIN, LOUD, NOISE, EXACT_MAX, QUIET, NOISE, NOISE),
         (EXACT_MIN, ZERO, NOISE, NOISE, LOUD, EXACT_MAX, QUIET, NOISE, NOISE))


def _pack(codes):
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, 4)
    return (c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]


def _window(rng, kind, table_type, nsample, nlow_min, nlow_max, sigma):
    """The bytes of one window of one digitiser."""
    if kind == ZERO:
        return np.zeros(nsample // 4, dtype=np.uint8)
    scale = {LOUD: 8.0, QUIET: 0.125}.get(kind, 1.0)
    while True:
        x = rng.standard_normal(nsample) * sigma * scale
        negative, high = x < 0, np.abs(x) >= THRESHOLD
        n_low = int((~high).sum())
        want = {EXACT_MIN: nlow_min, EXACT_MAX: nlow_max}.get(kind)
        if kind == LOUD and n_low >= nlow_min:
            want = nlow_min - 1                                   # (short windows: the draw alone does not always leave the limits)
        if kind == QUIET and n_low <= nlow_max:
            want = nlow_max + 1
        if want is not None:                                      # move samples across the threshold until n_low is `want`
            order = rng.permutation(nsample)
            for i in order:
                if n_low == want:
                    break
                if n_low > want and not high[i]:
                    high[i] = True
                    n_low -= 1
                elif n_low < want and high[i]:
                    high[i] = False
                    n_low += 1
            assert n_low == want
        if kind == NOISE and not nlow_min <= n_low <= nlow_max:
            continue                                              # noise windows are kept ones: the excised windows are the chosen ones
        data = _pack([code_of(table_type, bool(n), bool(h)) for n, h in zip(negative, high)])
        if not data.any():                                        # (an all-zero window is the ZERO kind's cause alone)
            negative[0] = not negative[0]
            data = _pack([code_of(table_type, bool(n), bool(h)) for n, h in zip(negative, high)])
        return data


def stream(table_type, npol, nsample, seed=0, kinds=KINDS, threshold=THRESHOLD):
    """A case's block of len(kinds[0]) whole windows: (block uint8, nlow_min, nlow_max).  The noise windows' sigma walks 0.8 ... 1.25,
    so that their n_low, and with it the level pair, differs from window to window."""
    rng = np.random.default_rng(1000 * seed + 100 * table_type + 10 * npol + nsample)
    nlow_min, nlow_max = limits_restated(nsample, threshold)
    nwindow = len(kinds[0])
    nbyte = nsample // 4
    block = np.zeros(nwindow * nbyte * npol, dtype=np.uint8)
    for idig in range(npol):
        for w, kind in enumerate(kinds[idig]):
            sigma = 0.8 + 0.45 * ((3 * w + idig) % nwindow) / (nwindow - 1)
            data = _window(rng, kind, table_type, nsample, nlow_min, nlow_max, sigma)
            block[idig + (w * nbyte) * npol:idig + ((w + 1) * nbyte) * npol:npol] = data
    return block, nlow_min, nlow_max


NSAMPLES = (4, 8, 64, 512)
CASES = [(t, npol, nsample) for t in TABLE_TYPES for npol in (1, 2) for nsample in NSAMPLES]


def case_id(case):
    return "%s-npol%d-n%d" % (("ob", "sm", "tc")[case[0]], case[1], case[2])
