"""The fused search epilogue on the four Coherence products (dspsr_amd/csrc: fb_search_fits in filterbank.hip, ts_part / ts_stage /
ts_reduce in fb_common.h, k_inv_chan<., 18 | 22, .> and k_rows_inv<., ., 4>) restated on the host, and the cases of
tests/test_gpu_coherence_search.py built from it.  Kept free of torch so that tests/test_coherence_search_cases_host.py can check on
a machine without a GPU that every case reaches the edge it is there for.

The staged tile of a workgroup is the exchange buffer of its transform: 2 * threads * 32 floats, the complex tile of T3 channels x 2
polarisations x freq_res bins.  The Coherence form stages FOUR floats per (channel, kept sample) as rows [channel * 4 + q][element of
the scrunch group][group] with G groups per row (G odd, at least the most groups a part can touch), so it fits where
tscrunch * G <= freq_res.  A tile has 4 * T3 rows on freq_res * T3 / 16 threads: 64 / freq_res rows per thread, each of which has one
carry -- the open output sample's partial sum -- that the thread reads before any thread of the workgroup replaces one."""
from collections import namedtuple

import numpy as np

NPO = 4                                   # rows per channel: PP, QQ, Re PQ*, Im PQ*
PTS = 32                                  # points per thread of a tile pass (csrc/wgfft.h)
SCALE = 0.0123                            # of the 8-bit samples
NCU = 256                                 # compute units of an MI355X: the inverse pass launches at most one workgroup each on a full tile


def tile(C, M):
    """(log2 of the channels per tile T3, threads of the inverse-pass workgroup) of the three-pass geometry of C channels of freq_res
    M: tiles of at most 2^14 points, M bins x (channel, polarisation) columns (csrc/filterbank.hip fb_tile).  The two-pass path's
    tile (k_rows_inv: Fb = 2^13 / M channels, 512 threads) is the same wherever it is taken."""
    logM = M.bit_length() - 1
    logT3 = min(C.bit_length() - 1, 13 - logM)
    return logT3, (M << logT3 << 1) // PTS


def groups(nkeep, sf):
    """G of fb_search_fits: groups per staged row"""
    return ((nkeep + 2 * sf - 2) // sf) | 1


def carries_per_thread(M):
    """TS_NPRE of the Coherence instantiation of freq_res M: a single-stage transform (freq_res <= 16) pre-loads up to four carries
    behind its only barrier, two stages at freq_res 32 load two in the stage hook, from freq_res 64 on one"""
    return 4 if M <= 16 else 2 if M == 32 else 1


def fits(C, M, nkeep, sf, npo=NPO):
    """fb_search_fits for a power-of-two three- or two-pass geometry with a scalar response (four passes, odd factors and the matrix
    response are refused before any of this)."""
    if M > 8192 or nkeep >= 65536 or sf >= 32768:
        return False
    logT3, nthr = tile(C, M)
    nrow = npo << logT3
    if nrow * sf * groups(nkeep, sf) > 2 * nthr * PTS or nrow > 4 * nthr or (nkeep + sf) * sf >= 2 ** 32:
        return False
    return npo != NPO or nrow <= carries_per_thread(M) * nthr


def rows_per_thread(C, M):
    logT3, nthr = tile(C, M)
    return -(-(NPO << logT3) // nthr)


def parts_of(nkeep, sf, parts):
    """TsPart (ts_part) of every part of a call sequence: (call, phase0, phi, ng, rlast) -- phase0 the carried samples when the call
    begins, phi the part's first sample within its first scrunch group, ng the groups it touches, rlast the samples it holds of the
    last one."""
    out, cc = [], 0
    for c, npart in enumerate(parts):
        for p in range(npart):
            s = cc + p * nkeep
            phi = s % sf
            e = phi + nkeep
            ng = -(-e // sf)
            out.append((c, cc, phi, ng, e - (ng - 1) * sf))
        cc = (cc + npart * nkeep) % sf
    return out


# A case: `real` dual-polarisation 8-bit input through setup(C, M, pos, neg, 1, 2, True, kernel, max_parts=maxp) with a random-phase
# unit kernel, or (real False) the complex geometry of test_gpu_search._fb_case(nchan=C, freq_res=M, dm, False, maxp), whose nfilt
# the Dedispersion response gives: `nkeep` is then what the test asserts of the engine, and npass the passes it must run -- both complex
# geometries would take the two-pass path (k_rows_inv) on an 8-bit block; j is there for k_inv_chan's form that is not pre-split,
# so its object is set up with force_four_pass = 2 (never the two-pass path) and runs three.  sfs: the scrunch factors run; fused[k]
# whether factor sfs[k] runs inside the inverse pass; rpt: carries per thread; carry: some part must read AND replace a carry and some
# call must begin inside a group; split: some call must be cut into launch groups (all three at the first factor).
Case = namedtuple("Case", "name C M nfilt nkeep real dm sfs fused parts maxp rpt carry split split_in_inverse npass what")


def _real(name, C, M, nfilt, sf, fused, parts, maxp, rpt, carry, split, what, split_in_inverse=False):
    return Case(name, C, M, nfilt, M - sum(nfilt), True, None, (sf,), (fused,), parts, maxp, rpt, carry, split, split_in_inverse, 3, what)


CASES = [
    _real("a", 128, 64, (9, 6), 5, True, (3, 5, 7), 2, 1, True, True, "fits; 512 staged rows on 512 threads"),
    # freq_res 32 and 16 are fused: two carries per thread loaded in the stage hook, four behind the single stage
    _real("b", 256, 32, (5, 4), 3, True, (5, 3, 7), 2, 2, True, True, "two rows per thread, two stages"),
    _real("c", 512, 16, (2, 1), 3, True, (5, 3, 7), 2, 4, True, True, "four rows per thread, single stage"),
    _real("d", 1024, 8, (2, 1), 3, False, (5, 3, 7), 2, 8, True, True, "4096 rows > 4 x 512 threads: not fused, results must still hold"),
    _real("e", 16, 2048, (300, 211), 7, True, (4, 4), 8, 1, True, False, "full-size tile, T3 = 4"),
    _real("f", 4, 256, (40, 30), 6, True, (3, 2), 4, 1, False, False, "a tile smaller than the full size: the LOGT = -1 instantiation"),
    _real("g", 8, 4096, (2000, 1000), 1200, True, (2, 3, 1), 2, 1, True, True, "a factor longer than a part: groups span parts and calls"),
    _real("h", 32, 1024, (335, 346), 1, True, (3, 2), 2, 1, False, True, "tscrunch 1: the products themselves, no carry read or written"),
    _real("i", 64, 1024, (3, 2), 16, False, (3, 2), 4, 1, True, False, "Coherence does not fit where PPQQ does"),
    Case("j", 128, 512, None, 500, False, 20.0, (7, 16), (True, False), (6, 2, 5), 4, 1, True, True, False, 3,
         "complex input on the three-pass path: the form that is not pre-split"),
    Case("k", 512, 512, None, 508, False, 100.0, (2, 16), (True, False), (3, 2), 8, 1, False, False, False, 2, "the two-pass path (k_rows_inv)"),
    _real("m", 1024, 4096, (2000, 1000), 7, True, (2, 1), 2, 1, True, False,
          "512 tiles, more than the chip has compute units: a workgroup walks the parts of several tiles, one after the other"),
    _real("l", 64, 256, (41, 30), 6, True, (3, 4, 2), 3, 1, True, True, "real input with the split in the inverse pass: not pre-split",
          split_in_inverse=True),
]
BY_NAME = {c.name: c for c in CASES}


def kernel_of(case):
    """the random-phase unit response of a real case"""
    rng = np.random.default_rng(1000 * case.M + case.sfs[0])
    return np.exp(1j * rng.uniform(-np.pi, np.pi, case.C * case.M)).astype(np.complex64)


def raw_block(rng, nsamp, real):
    """nsamp 8-bit samples of two polarisations (complex: interleaved re, im)"""
    return np.clip(np.rint(rng.standard_normal(nsamp * 2 * (1 if real else 2)) * 24.0), -128, 127).astype(np.int8)
