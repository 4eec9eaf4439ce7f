"""The case tables of the spectral-kurtosis tests (tests/test_sk_cases_host.py proves on the restatement alone that every case reaches
its edge; tests/test_gpu_sk.py runs them on the device).

EXACT data are small integers: every sample is s * t with t in {-1, 0, +1}, P(t != 0) = 1/3 -- a distribution whose kurtosis is 3, as a
Gaussian's, so that the estimates scatter about 1 -- and s an integer scale per channel, at most 4 (doubled where a feature asks, so
|re|, |im| <= 8).  The scale is bounded so that npart * M * max(|x|^4) <= 2^24: every S1, S2 and tscr sum is an integer below 2^24,
exact in float32 in any order of addition (exact_bound)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sk_limits.json")

# name: M nchan npol npart rem std_devs (chan_start, chan_end) (no_fscr, no_tscr, no_ft) offset pad features expect
#   rem      samples behind the last whole part (never touched)
#   offset   floats the rows start behind a 16-byte boundary (0: 16-byte aligned, 2: 8-byte aligned)
#   pad      spare floats per row (padded strides)
#   features const: (part, chan) of constant modulus (estimate 0: an skfb zap);  zero: (part, chan) of zeros (S1 == 0);
#            tscr: channels whose odd parts are twice as strong (each part clean, the whole call not);
#            fscr: parts whose first max(1, M // 32) samples are twice as strong in every channel (each channel clean, their mean not)
#   expect   the edges the host test must find reached on the restatement
EXACT = {
    "m128_c64_p2_n64": dict(M=128, nchan=64, npol=2, npart=64, rem=0, offset=0, pad=0,
                            const=[(3, 0), (5, 63)], zero=[(7, 10)], tscr=[20], fscr=[11, 40],
                            expect={"tscr", "skfb_first", "skfb_last", "fscr_only", "s1_zero"}),
    "m128_c64_p2_n7_range": dict(M=128, nchan=64, npol=2, npart=7, rem=1, offset=2, pad=6, chans=(4, 60),
                                 const=[(1, 4), (1, 5), (2, 59), (2, 60), (3, 0), (3, 63), (5, 30)], fscr=[5],
                                 expect={"skfb_borders", "fscr_after_zaps", "skfb_first", "skfb_last"}),
    "m32_c257_p1_n64": dict(M=32, nchan=257, npol=1, npart=64, rem=31, offset=0, pad=4,
                            const=[(0, 0), (63, 256)], zero=[(10, 100)], fscr=[20],
                            expect={"skfb_first", "skfb_last", "s1_zero", "fscr_only"}),
    "m33_c3_p2_n7_range": dict(M=33, nchan=3, npol=2, npart=7, rem=0, offset=0, pad=0, chans=(1, 2), const=[(2, 1)], expect=set()),
    "m33_c64_p1_n2": dict(M=33, nchan=64, npol=1, npart=2, rem=32, offset=2, pad=4, fscr=[1], expect={"fscr_only"}),
    "m100_c1_p2_n1": dict(M=100, nchan=1, npol=2, npart=1, rem=1, offset=0, pad=0, expect=set()),
    "m100_c3_p1_n64": dict(M=100, nchan=3, npol=1, npart=64, rem=99, offset=2, pad=0, tscr=[1], expect={"tscr"}),
    "m1000_c3_p2_n2": dict(M=1000, nchan=3, npol=2, npart=2, rem=0, offset=2, pad=10, const=[(1, 2)], expect={"skfb_last"}),
    "m1000_c64_p1_n7_no_tscr": dict(M=1000, nchan=64, npol=1, npart=7, rem=1, offset=0, pad=0, flags=(False, True, False), fscr=[3],
                                    tscr=[9], expect={"fscr_only", "no_tscr"}),
    "m1024_c3_p2_n64": dict(M=1024, nchan=3, npol=2, npart=64, rem=0, offset=0, pad=4, tscr=[1], expect={"tscr"}),
    "m1024_c257_p1_n1": dict(M=1024, nchan=257, npol=1, npart=1, rem=1023, offset=0, pad=0, const=[(0, 256)], expect={"skfb_last"}),
    "m128_c64_p2_n7_no_fscr": dict(M=128, nchan=64, npol=2, npart=7, rem=0, offset=0, pad=0, flags=(True, False, False), fscr=[2],
                                   expect={"no_fscr"}),
    "m128_c64_p1_n7_no_ft": dict(M=128, nchan=64, npol=1, npart=7, rem=0, offset=2, pad=2, flags=(False, False, True), const=[(1, 5)],
                                 expect={"no_ft"}),
    "m128_c1_p1_n2": dict(M=128, nchan=1, npol=1, npart=2, rem=127, offset=2, pad=0, expect=set()),
    "m1024_c3_p1_n2_6sigma": dict(M=1024, nchan=3, npol=1, npart=2, rem=0, offset=0, pad=0, std_devs=6, const=[(0, 1)], expect=set()),
    "m128_c64_p2_n2_1sigma": dict(M=128, nchan=64, npol=2, npart=2, rem=0, offset=0, pad=0, std_devs=1, expect=set()),
}
IDS = sorted(EXACT)
EDGES = {"tscr", "skfb_first", "skfb_last", "skfb_borders", "fscr_after_zaps", "fscr_only", "s1_zero", "no_fscr", "no_tscr", "no_ft"}

# the values the issue asks the shapes to take
WANT_M, WANT_NCHAN, WANT_NPART = {32, 33, 100, 128, 1000, 1024}, {1, 3, 64, 257}, {1, 2, 7, 64}


def case(name):
    c = dict(std_devs=3, chans=(0, 0), flags=(False, False, False), const=[], zero=[], tscr=[], fscr=[])
    c.update(EXACT[name])
    c["name"] = name
    c["ndat"] = c["npart"] * c["M"] + c["rem"]
    return c


def scale_limit(c):
    """The largest integer scale s <= 4 with npart * M * (2 * (2s)^2)^2 <= 2^24 (a doubled sample has |re|, |im| = 2s)."""
    s = 4
    while s > 1 and c["npart"] * c["M"] * (8 * s * s) ** 2 > 2 ** 24:
        s -= 1
    return s


def exact_bound(c, rows):
    """|re|, |im| <= 8 and the sum of |x|^4 over all parts of any row stays below 2^24: every float32 sum of the case is exact."""
    x = rows[:, :, :2 * c["npart"] * c["M"]].astype(np.int64)
    p = x[..., 0::2] ** 2 + x[..., 1::2] ** 2
    return np.abs(rows).max() <= 8 and np.array_equal(rows, np.rint(rows)) and int((p * p).sum(axis=-1).max()) <= 2 ** 24


def exact_rows(c):
    """float32 [nchan][npol][2 * ndat]"""
    M, nchan, npol, npart, ndat = c["M"], c["nchan"], c["npol"], c["npart"], c["ndat"]
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    t = rng.choice(np.array([-1, 0, 0, 0, 0, 1], np.int64), size=(nchan, npol, ndat, 2))
    scale = 1 + (np.arange(nchan) % scale_limit(c))
    x = t * scale[:, None, None, None]
    for part, chan in c["const"]:
        x[chan, :, part * M:(part + 1) * M] = (scale[chan], -scale[chan])
    for part, chan in c["zero"]:
        x[chan, :, part * M:(part + 1) * M] = 0
    for chan in c["tscr"]:
        for part in range(1, npart, 2):
            x[chan, :, part * M:(part + 1) * M] *= 2
    for part in c["fscr"]:
        x[:, :, part * M:part * M + max(1, M // 32)] *= 2
    return np.ascontiguousarray(x.reshape(nchan, npol, 2 * ndat).astype(np.float32))


def golden_limits():
    """{(M, std_devs): row} of tests/golden/sk_limits.json: the table of the reference's own dsp::SKLimits."""
    with open(GOLDEN) as f:
        return {(r["M"], r["std_devs"]): r for r in json.load(f)["rows"]}


def limits_of(c, npart=None):
    """(lower, upper) for M and for M * npart, as SpectralKurtosis takes them from dsp::SKLimits (the product's port of it, which
    tests/test_sk_limits_host.py holds to the reference's table)."""
    import dspsr_amd
    m_t = int(np.float32(c["M"] * (c["npart"] if npart is None else npart)))          # SpectralKurtosis.C:472,493: M_tscr = float(m)
    return dspsr_amd.sk_limits(c["M"], c["std_devs"]), dspsr_amd.sk_limits(m_t, c["std_devs"])


def detector(c):
    import sk_reference as ref
    return ref.Detector(c["nchan"], c["npol"], c["M"], c["std_devs"], c["chans"][0], c["chans"][1], *c["flags"])


def staged(c, est, est_tscr, limits, limits_tscr, det=None):
    """SpectralKurtosis::detect step by step on the restatement; the mask after every step.  -> detector, {step: mask}"""
    det = det or detector(c)
    masks = {}
    det.reset_mask(est.shape[0])
    if not det.no_tscr:
        det.detect_tscr(est_tscr, *limits_tscr)
    masks["tscr"] = det.mask.copy()
    if not det.no_ft:
        det.detect_skfb(est, *limits)
    masks["skfb"] = det.mask.copy()
    if not det.no_fscr:
        det.detect_fscr(est)
    masks["fscr"] = det.mask.copy()
    det.count_zapped(est)
    return det, masks


# random float rows: (M, nchan, npol, npart, rem)
NOISE = [(32, 5, 2, 9, 3), (33, 3, 1, 5, 0), (128, 16, 2, 64, 0), (1000, 3, 2, 3, 7), (1024, 4, 1, 8, 0), (65536, 1, 2, 2, 0)]


def noise_rows(index):
    M, nchan, npol, npart, rem = NOISE[index]
    rng = np.random.default_rng(100 + index)
    x = rng.normal(size=(nchan, npol, 2 * (npart * M + rem))) * (1 + np.arange(nchan))[:, None, None]
    x[0, :, :2 * M:16] *= 6                                    # some strong samples in the first part of the first channel
    return x.astype(np.float32)


def chain_length(M):
    """L(M) of k_sk_compute (csrc/sk.hip): the longest chain of additions a term of S1 or S2 passes through."""
    P = (M + 1) // 2
    W = 16 if P <= 64 else 32 if P <= 128 else 64
    pairs_per_lane = -(-P // W)
    return 2 * -(-pairs_per_lane // 4) - 1 + 2 + (W.bit_length() - 1)
