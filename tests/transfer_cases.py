"""The filterbank's response measured bin by bin (tests/test_gpu_transfer.py, tests/test_transfer_cases_host.py): the inputs, the float64
truth, the float32 baseline, the measure and the case table as plain data and numpy.  No torch.

The measurement.  The input of a case is PERIODIC with period nsamp_fft.  Part p of the overlap-save loop starts p * nsamp_step samples
in and so sees the period circularly shifted; nsamp_step / nsamp_fft = nkeep / M (M = freq_res) for real and complex input alike, so
the shift multiplies bin k = c M + m of the part's spectrum by exp(2 pi i m p nkeep / M) and output sample t = p nkeep + j of channel c is

    y_c[t] = sum_m X[c M + m] kernel[c M + m] exp(2 pi i m (t + nfilt_pos) / M)                (X: the transform of one period)

-- one M-periodic series over all parts.  The M-point DFT (host, float64, divided by M) of any M contiguous samples from t0 on is

    G[c M + m] = X[k] kernel[k] exp(2 pi i m (t0 + nfilt_pos) / M)

the complex gain of every bin, one number per bin: a defect of relative size d at bin k is d at G[k], undiluted, where the time-domain
comparison of test_gpu_parity._fb_case sees d / sqrt(M); rounding noise spreads evenly.  The periods have unit-modulus bins, so "relative
to the rms amplitude" and "relative to the bin" agree (to 5 % after rounding to 8 bits; test_transfer_cases_host.py holds the factor).

The table.  filterbank.hip picks every kernel from a few integers (fb_tile, fb_takes_presplit, fb_pick_kernels, fb_setup_two_pass,
fb_setup_conv, fb_pass1): `picks` restates them, `reachable` enumerates what a call with L <= 2^22 and freq_res <= 2^17 can reach,
and the table holds for every reachable tuple the smallest transform that reaches it.  Tuples:
    ("p1", logM, raw width, full, pre-split)       k_fwd_cols / k_fwd_cols_rm           ("p1d",): k_fwd_cols_dual
    ("p2", logR, full, pre-split)                  k_fwd_rows / k_fwd_rows_split
    ("p3", logM, full, pre-split, real)            k_inv_chan (real: the mirror loads; full, logM 12, real, not pre-split: pair16)
    ("p3a", logMa, blocked, real, full)            k_inv_a        ("p3b", logMb, full)    k_inv_b
    ("rinv", logM) ("p1t", lfa, full) ("col1q",)   the two-pass path: k_rows_inv and its pass 1
PINNED names every instantiation outside that set with the reason."""
import functools
import math

import numpy as np

import fused_fold_cases as ffc
import matrix_cases

MAX_LOGF, LOG_POINTS, PTS = ffc.MAX_LOGF, ffc.LOG_POINTS, ffc.PTS
ODD_MAX = ffc._constant("fb_common.h", "ODD_MAX")
CONV3_MIN_LOGM, CONV3_MAX_LOGM = 14, 21       # fb_common.h
MAX_LOG_L, MAX_LOG_FRES = 22, 17              # the lengths the table goes to (the headline's transform; cfg 1's freq_res and a step beyond)
NPART, MAX_PARTS = 3, 2                       # a call of a full launch group and a ragged one
RMS8 = 24.0                                   # counts per unit of `period`: 17 counts rms (real), 12 per component (complex)


def _ilog2(v):
    n = int(v).bit_length() - 1
    assert v > 0 and 1 << n == v, v
    return n


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def _odd_part(v):
    while v and not v & 1:
        v >>= 1
    return v


def _radix_ok(r):
    return r & 1 and 3 <= r <= ODD_MAX


def _full_logt(logf):
    return 14 - logf if 14 - logf >= 1 else -1


def default_nfilt(M):
    """nkeep >= M / 2, both sides unequal, nfilt_pos >= 1 where freq_res has room for it"""
    if M == 1:
        return (0, 0)
    pos, neg = max(1, M // 5), M // 7
    assert M - pos - neg >= (M + 1) // 2
    return (pos, neg)


# ---- the host's choice of kernels, restated ----------------------------------------------------------------------------------------
def picks(C, M, real, npol=2, form="raw8", input_nchan=1, four=0, sii=False, matrix=False, nfilt=None):
    """What dspsr_amd_filterbank_create and one perform call of complex rows choose for this object and this input form ("raw8": the
    generic 8-bit block, "caspsr", "float": float32 rows), at the allocator's alignment with dense rows.  None: create refuses.
    A dict: path, passes (what npass() answers for this form), presplit, L, tuples (see the module text)."""
    nfilt = default_nfilt(M) if nfilt is None else nfilt
    nkeep = M - sum(nfilt)
    if form == "caspsr" and not (real and npol == 2 and input_nchan == 1):
        return None
    if M == 1:                                                               # fb_create_plain
        if not (_pow2(C) and 2 <= C <= 1 << MAX_LOGF) or four:
            return None
        return dict(path="plain", passes=1, npass=1, presplit=False, L=(2 if real else 1) * C, tuples=(("plain", _ilog2(C), real, npol),))
    # fb_check_factors
    msub = 0
    if not _pow2(M):
        msub = _odd_part(M)
        if not (_radix_ok(msub) and (_pow2(C) or _radix_ok(_odd_part(C) * msub)) and M // msub >= 2 and four != 1):
            return None
    nchan_sb, fres = (C * msub, M // msub) if msub else (C, M)
    nsub = 1
    if not _pow2(nchan_sb):
        nsub = _odd_part(nchan_sb)
        if not _radix_ok(nsub) or four == 1:
            return None
    if sum(nfilt) >= M:
        return None
    # fb_init_geom
    N = nchan_sb * fres
    L = 2 * N if real else N
    logMf = logM = _ilog2(fres)
    logR = _ilog2(L // nsub // fres)
    logC = _ilog2(nchan_sb // nsub)
    logL = logM + logR
    # fb_tile
    three = logM <= MAX_LOGF and logR <= MAX_LOGF
    logT1 = logT2 = logT3 = logX3 = 0
    if three:
        logT1, logT2 = min(logR, LOG_POINTS - logM), min(logM, LOG_POINTS - logR)
        logX3 = logT3 = min(logC, max(0, LOG_POINTS - logM - 1))
        p1, p2, p3 = fres << logT1, (1 << logR) << logT2, (fres << logT3) << 1
        three = not (p1 < 32 or p2 < 32 or p3 < 32 or p3 > 1 << LOG_POINTS or logT1 < 1 or logT2 < 1)
    if nsub > 1 and not three:
        return None
    four_pass = four == 1 or not three
    xblocked = False
    if four_pass:
        la = min((logL + 1) // 2, MAX_LOGF)
        lb = logL - la
        blocked = min(la, LOG_POINTS - lb) < 4
        lma_best = (0,) * 14 + (6, 7, 8, 9, 10, -1, 10, 11, 11, 11, 12, 12, 13)
        lma = (logMf + 1) // 2
        if 14 <= logMf <= 26:
            lma = lma_best[logMf] if lma_best[logMf] > 0 else (11 if blocked else 9)
        lma = min(lma, MAX_LOGF)
        lmb = logMf - lma
        logM, logR, logT3, logX3 = la, lb, 0, 0
        logT1, logT2 = min(lb, LOG_POINTS - la), min(la, LOG_POINTS - lb)
        logTm, logTt = min(lmb, LOG_POINTS - 1 - lma), min(lma, LOG_POINTS - 1 - lmb)
        p1, p2 = (1 << la) << logT1, (1 << lb) << logT2
        p3, p4 = ((1 << lma) << logTm) << 1, ((1 << lmb) << logTt) << 1
        if not (1 <= lb <= MAX_LOGF and 1 <= lmb <= MAX_LOGF and logT1 >= 1 and logT2 >= 1 and logTm >= 0 and logTt >= 0 and
                min(p1, p2, p3, p4) >= 32):
            return None
        xblocked = blocked and lmb >= logT2 and p3 // PTS >= 1 << logT2
    # fb_pick_kernels
    full1, full2 = logT1 == _full_logt(logM), logT2 == _full_logt(logR)
    full3 = not four_pass and logT3 + 1 == _full_logt(logM)
    dual = full1 and logM == 13 and logT1 == 1 and logT1 + logT2 < 4 and logR >= 2
    ps = not sii and real and npol == 2 and nsub == 1 and not msub and not four_pass and not dual and 1 <= logT2 <= logM
    rec = dict(L=L, presplit=ps, nsub=nsub, msub=msub, logM=logM, logR=logR, logT2=logT2, logX3=logX3)
    # set_response_matrix (npol 2, one input channel, three passes, power-of-two lengths)
    if matrix and (npol != 2 or input_nchan != 1 or four_pass or nsub > 1 or msub or C == 1 or M > 8192):
        return None
    # fb_setup_conv and the dispatcher's order
    conv = C == 1 and not real and npol == 2 and not msub and nsub == 1
    if conv and form == "float" and four == 0 and 6 <= logMf <= 13:
        return dict(rec, path="conv1", passes=1, npass=1, tuples=(("conv1", logMf),))
    if conv and form == "float" and four == 0 and CONV3_MIN_LOGM <= logMf <= CONV3_MAX_LOGM:
        return dict(rec, path="conv3", passes=3, npass=3, tuples=(("conv3", logMf),))
    if (conv and form == "float" and input_nchan >= 4 and four != 2 and four_pass and not xblocked and
            not (logR >= 6 and logT1 <= 4)):
        ch = 1
        while ch < 64 and input_nchan % (2 * ch) == 0:
            ch *= 2
        while ch > 1 and _ilog2(ch) + logMf > 21:
            ch //= 2
        if ch >= 2:
            return dict(rec, path="batched", passes=4, npass=4, tuples=(("batched", logMf, ch),))
    # fb_setup_two_pass / fb_takes_two_pass
    step = (2 if real else 1) * C * nkeep                                    # nsamp_step, the input's part step in samples
    lfb, lfa = 13 - logMf, _ilog2(L // nsub) - (13 - logMf) if nsub == 1 else 0
    two_obj = (nsub == 1 and not four_pass and not real and npol == 2 and four != 2 and 9 <= logMf <= 12 and logMf <= lfa <= 14)
    q_logT1 = min(lfb, LOG_POINTS - lfa)
    if two_obj and lfa < 14 and not (q_logT1 >= 1 and (1 << lfa) << q_logT1 >= 32):
        two_obj = False
    # (npass() answers for the object and the kind of input; the call also wants whole words and, below Fa = 2^14, one input channel)
    rec["npass"] = 2 if two_obj and form != "float" and not matrix else 4 if four_pass else 3
    if two_obj and not matrix and form == "raw8" and step % 4 == 0 and (lfa == 14 or input_nchan == 1):
        pass1 = ("col1q",) if lfa == 14 else ("p1t", lfa, q_logT1 == _full_logt(lfa))
        return dict(rec, path="two", passes=2, lfa=lfa, tuples=(pass1, ("rinv", logMf)))
    # fb_pass1 (power-of-two geometries; the sub-band path feeds pass 1 sub-sequences of its own and stays out of the tuples)
    if nsub > 1 or msub:
        return dict(rec, path="odd", passes=4 if four_pass else 3, tuples=())
    raw8 = form in ("raw8", "caspsr")
    fast8 = raw8 and real and npol == 2 and input_nchan == 1
    fastc = form == "raw8" and not real and npol == 2 and input_nchan == 1 and step % 4 == 0 and logR >= 3
    regroup = (fast8 or fastc) and logR >= 2 and logT1 <= 5
    if regroup and form == "caspsr" and step % 4:
        regroup = False
    raww = 1 if regroup or (fast8 and form == "raw8") else 4
    if dual and raww != 1:
        dual = False                                                         # (fb_pick1_dual(4) is null: the call keeps k_fwd_cols)
    tuples = [("p1d",) if dual else ("p1", logM, raww, full1, ps), ("p2", logR, full2, ps)]
    if four_pass:
        tuples += [("p3a", lma, xblocked, real, logTm == 13 - lma and lma <= 12 and p3 // PTS == 512),
                   ("p3b", lmb, logTt == 13 - lmb and lmb <= 12 and p4 // PTS == 512)]
    else:
        tuples += [("p3m" if matrix else "p3", logMf, full3, ps, real)]
    return dict(rec, path="tiles", passes=4 if four_pass else 3, tuples=tuple(tuples))


def _universe():
    """every call the enumeration considers: power-of-two lengths, both input kinds, one and two polarisations, 8-bit blocks and
    float rows, the split in either pass, the four-pass form forced or not"""
    for logM in range(1, MAX_LOG_FRES + 1):
        for real in (True, False):
            for logC in range(0, MAX_LOG_L - logM - (1 if real else 0) + 1):
                for npol in (2, 1):
                    for form in ("raw8", "float"):
                        for sii in ((False, True) if real and npol == 2 else (False,)):
                            for four in (0, 1):
                                yield dict(C=1 << logC, M=1 << logM, real=real, npol=npol, form=form, sii=sii, four=four)


@functools.lru_cache(maxsize=None)
def reachable():
    """{tuple: the call with the smallest transform that reaches it (ties: two polarisations, the 8-bit block, no force; at
    L = 2^22 one polarisation -- no tuple of that length depends on npol, and the float64 truth of two takes a host 9 s)}"""
    best = {}
    for kw in _universe():
        r = picks(**kw)
        if r is None or r["path"] != "tiles":
            continue
        rank = (r["L"], kw["npol"] != (1 if r["L"] >> MAX_LOG_L else 2), kw["form"] != "raw8", kw["four"], kw["sii"])
        for t in r["tuples"]:
            if t not in best or rank < best[t][0]:
                best[t] = (rank, kw)
    return {t: dict(kw) for t, (rank, kw) in best.items()}


def instantiated():
    """every tuple the kernel tables of fb_fwd_cols.hip, fb_fwd_cols_rm.hip, fb_fwd_rows.hip, fb_inv_chan.hip and fb_four_pass.hip hold
    at a length of 2 ... 2^13 (pre-split: real input only)"""
    tf = (False, True)
    out = {("p1d",)}
    for logf in range(1, MAX_LOGF + 1):
        out |= {("p1", logf, w, full, ps) for w in (1, 4) for full in tf for ps in tf}
        out |= {("p2", logf, full, ps) for full in tf for ps in tf}
        out |= {("p3", logf, full, ps, real) for full in tf for ps in tf for real in tf if real or not ps}
        out |= {("p3a", logf, xb, real, full) for xb in tf for real in tf for full in tf}
        out |= {("p3b", logf, full) for full in tf}
    return out


def _pinned():
    """The instantiations no call with L <= 2^22 and freq_res <= 2^17 reaches, each group with its reason."""
    tf = (False, True)
    pin = {}

    def add(reason, tuples):
        for t in tuples:
            assert t not in pin, t
            pin[t] = reason
    add("k_fwd_cols_dual: freq_res 2^13 and a pass-2 tile of at most four rows, logR >= 12 -- L >= 2^25",
        [("p1d",)])
    add("2^13-point columns and rows: the tile of two (logT = 1 = full_logt(13)) is the full tile, the generic form is never picked",
        [("p1", 13, w, False, ps) for w in (1, 4) for ps in tf] + [("p2", 13, False, ps) for ps in tf] +
        [("p3", 13, False, ps, real) for ps in tf for real in tf if real or not ps])
    add("complex input, freq_res 4096: the generic tile is one channel, and one channel of complex input (logR = 0) has no three-pass form",
        [("p3", 12, False, False, False)])
    add("freq_res 2 and 4 have no four-pass form (the second inverse pass would hold fewer than 32 points)",
        [("p3a", 1, xb, real, full) for xb in tf for real in tf for full in tf] + [("p3b", 1, full) for full in tf])
    add("a full tile of the inverse passes needs logMa + logMb >= 13: forced at freq_res 8192 (logMa 7, logMb 6) or by length",
        [("p3a", lma, xb, real, True) for lma in (2, 3, 4, 5) for xb in tf for real in tf] + [("p3b", lmb, True) for lmb in (2, 3, 4, 5)])
    add("a blocked spectrum (L = 2^22, pass-2 tiles of 8 rows) needs logMb >= 3 and 256 points in the first inverse tile",
        [("p3a", lma, True, real, False) for lma in (2, 3) for real in tf])
    add("logMa 7, 8, 9 come with logMb >= 13 - logMa (freq_res 8192 forced, 2^15, 2^16, 2^17): always the full tile",
        [("p3a", lma, xb, real, False) for lma in (7, 8, 9) for xb in tf for real in tf])
    add("logMb 8 comes with logMa >= 6 (freq_res 2^14 ... 2^17): always the full tile",
        [("p3b", 8, False)])
    add("lma_best of fb_tile: logMa >= 10 from freq_res 2^18 on, logMb >= 10 from 2^19 on, logMb 7 and 9 at no freq_res",
        [("p3a", lma, xb, real, full) for lma in (10, 11, 12, 13) for xb in tf for real in tf for full in tf] +
        [("p3b", lmb, full) for lmb in (7, 9, 10, 11, 12, 13) for full in tf])
    return pin


PINNED = _pinned()


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def make_case(family, C, M, real, npol=2, form="raw8", input_nchan=1, four=0, sii=False, matrix=False, kernel=True, npart=NPART,
          max_parts=MAX_PARTS):
    nfilt = default_nfilt(M)
    p = picks(C, M, real, npol, form, input_nchan, four, sii, matrix, nfilt)
    assert p is not None, (family, C, M, real, npol, form, input_nchan, four, sii, matrix)
    name = "%s-%dx%d-%s%d-%s" % (family, C, M, "r" if real else "c", npol, form)
    name += ("-in%d" % input_nchan if input_nchan > 1 else "") + ("-four" if four else "") + ("-sii" if sii else "")
    name += ("-jones" if matrix else "") + ("" if kernel else "-nokernel")
    return dict(name=name, family=family, C=C, M=M, nfilt=nfilt, real=real, npol=npol, form=form, input_nchan=input_nchan, four=four,
                sii=sii, matrix=matrix, kernel=kernel, npart=npart, max_parts=max_parts, picks=p)


COMPILED_RADICES = (3, 5, 7, 9, 15)           # k_sub_combine<R> / k_time_combine<R>; every other odd factor: the run-time-radix forms
ODD_FACTORS = tuple(range(3, ODD_MAX + 1, 2))
ODD_PRODUCTS = ((3, 15), (5, 5), (3, 35))     # (factor of nchan_subband, factor of freq_res), as in tests/test_gpu_two_pass.py


def smallest_odd(rc, rm, real):
    """(C, M) of the shortest transform the library accepts with the odd factors rc of nchan_subband and rm of freq_res"""
    best = None
    for a in range(0, 10):
        for b in range(1, 12):
            C, M = rc << a, rm << b
            p = picks(C, M, real)
            if p is not None and (best is None or (p["L"], C) < best[0]):
                best = ((p["L"], C), C, M)
    assert best is not None, (rc, rm, real)
    return best[1], best[2]


def _cases():
    out, seen = [], set()

    def add(*a, **kw):
        c = make_case(*a, **kw)
        if c["name"] not in seen:
            seen.add(c["name"])
            out.append(c)
        return c
    # every reachable tuple at the smallest transform that reaches it, the longest first (they cover the most)
    reach = reachable()
    covered = set()
    for t in sorted(reach, key=lambda t: (-picks(**reach[t])["L"], str(t))):
        if t in covered:
            continue
        kw = reach[t]
        p = picks(**kw)
        covered |= set(p["tuples"])
        add("three" if p["passes"] == 3 else "four", **kw)
    # four passes by length at every freq_res 2^14 ... 2^17, both input kinds, beside what the cover took
    for logM in range(14, MAX_LOG_FRES + 1):
        add("four", 2, 1 << logM, True)
        add("four", 2, 1 << logM, False, form="float")
    # the other input forms of the three- and four-pass kernels
    add("three", 16, 256, True, form="caspsr")
    add("four", 16, 256, True, form="caspsr", four=1)
    add("three", 32, 128, False, npol=1)
    # two passes: freq_res 512 ... 4096, the fewest and the most channels each admits (lfa = 14: k_fwd_col1q)
    for logM in range(9, 13):
        for C in (1 << (13 - logM), 1 << (27 - 2 * logM)):
            c = add("two", C, 1 << logM, False)
            assert c["picks"]["path"] == "two" and (c["picks"]["lfa"] == 14) == (C == 1 << (27 - 2 * logM))
    # every odd factor once in nchan_subband and once in freq_res, input kinds alternating; the compiled radices with both
    for i, R in enumerate(ODD_FACTORS):
        for where in ("C", "M"):
            for real in ((True, False) if R in COMPILED_RADICES else ((i + (where == "M")) % 2 == 0,)):
                C, M = smallest_odd(R, 1, real) if where == "C" else smallest_odd(1, R, real)
                add("odd_" + where, C, M, real)
    for rc, rm in ODD_PRODUCTS:
        add("odd_CM", *smallest_odd(rc, rm, True), True)
    add("odd_CM", *smallest_odd(3, 15, False), False)
    # the other families at the shapes of tests/output_forms.FAMILIES
    add("subbands", 16, 256, True, input_nchan=2)
    add("subbands", 32, 128, False, input_nchan=4, form="float")
    add("plain", 64, 1, True, npart=70)
    add("plain", 64, 1, True, form="float", npart=70)
    for logM in range(6, 14):
        add("conv1", 1, 1 << logM, False, form="float", input_nchan=3)
    add("conv3", 1, 16384, False, form="float", input_nchan=3)
    add("conv3", 1, 131072, False, form="float", input_nchan=3, max_parts=512)
    add("batched", 1, 1024, False, form="float", input_nchan=4, four=1)
    # the matrix response (tests/matrix_cases.py): pre-split, the split in the inverse pass, a full tile, complex input, the
    # two-pass geometry (a matrix response keeps it on three passes)
    add("matrix", 16, 256, True, matrix=True)
    add("matrix", 16, 256, True, matrix=True, sii=True)
    add("matrix", 4, 4096, True, matrix=True)
    add("matrix", 2048, 16, True, matrix=True, form="float")
    add("matrix", 32, 128, False, matrix=True)
    add("matrix", 16, 512, False, matrix=True)
    # no response at all (kernel = NULL), once per family
    add("three", 16, 256, True, kernel=False)
    add("four", 16, 256, True, four=1, kernel=False)
    add("four", 2, 16384, True, kernel=False)
    add("two", 16, 512, False, kernel=False)
    add("odd_C", 96, 256, True, kernel=False)
    add("odd_M", 16, 640, True, kernel=False)
    add("subbands", 16, 256, True, input_nchan=2, kernel=False)
    add("plain", 64, 1, True, npart=70, kernel=False)
    add("conv1", 1, 4096, False, form="float", input_nchan=3, kernel=False)
    add("conv3", 1, 16384, False, form="float", input_nchan=3, kernel=False)
    add("batched", 1, 1024, False, form="float", input_nchan=4, four=1, kernel=False)
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]
EXPECTED_PATH = dict(three=("tiles",), four=("tiles",), two=("two",), odd_C=("odd",), odd_M=("odd",), odd_CM=("odd",),
                     subbands=("tiles",), plain=("plain",), conv1=("conv1",), conv3=("conv3",), batched=("batched",), matrix=("tiles",))


def by_name(name):
    return CASES[NAMES.index(name)]


def table_tuples():
    """the tuples the scalar-response cases of the three-, four- and two-pass families reach"""
    return {t for c in CASES if c["family"] in ("three", "four") and not c["matrix"] for t in c["picks"]["tuples"]}


# ---- periods, responses, blocks ------------------------------------------------------------------------------------------------------
def _seed(name, k=0):
    import zlib
    return (zlib.crc32(name.encode()) + k) & 0x7fffffff


def period(nsamp_fft, real, rng):
    """One period as float64 rows of nsamp_fft * ndim floats, the backward transform of unit-modulus random-phase bins scaled to a
    mean square of 1/2 per sample (real: rms 0.71; complex: 0.5 per component).  Real input: DC +1 and Nyquist -0.5 of that modulus -- both present and unequal, so a Hermitian split that
    let the Nyquist bin into bin 0 shows there."""
    n = nsamp_fft
    if real:
        X = np.exp(1j * rng.uniform(-np.pi, np.pi, n // 2 + 1))
        X[0], X[n // 2] = 1.0, -0.5
        return np.fft.irfft(X, n) * math.sqrt(n / 2.0)
    X = np.exp(1j * rng.uniform(-np.pi, np.pi, n))
    x = np.fft.ifft(X) * math.sqrt(n / 2.0)
    return np.ascontiguousarray(x).view(np.float64)


def make_plan(o, c):
    C, M, real = c["C"], c["M"], c["real"]
    N, (nfp, nfn) = C * M, c["nfilt"]
    plan = o.FilterbankPlan(C * c["input_nchan"], c["input_nchan"], C, M, N, nfp, nfn, nfp + nfn, 2 * N if real else N,
                            (2 if real else 1) * (nfp + nfn) * C, 0, M - nfp - nfn, float(N) * M, real)
    plan.nsamp_step = plan.nsamp_fft - plan.nsamp_overlap
    return plan


def block(o, c):
    """The input of a case (its dict): rows float32 [input_nchan][npol][ndat * ndim] (the periods tiled), raw (the int8 block they were unpacked
    from, or None for float rows), the response (`kernel` complex64 or None, `matrix8` float32 [N][8] or None), plan, obs, scale."""
    import types
    name = c["name"]
    plan = make_plan(o, c)
    real, npol, nin, form = c["real"], c["npol"], c["input_nchan"], c["form"]
    ndim = 1 if real else 2
    obs = o.Observation(nchan=nin, npol=npol, ndim=ndim, machine="CASPSR" if form == "caspsr" else "DADA")
    ndat = c["npart"] * plan.nsamp_step + plan.nsamp_overlap
    if form == "caspsr":
        ndat = -(-ndat // 4) * 4
    rng = np.random.default_rng(_seed(name))
    per = np.stack([[period(plan.nsamp_fft, real, rng) for _ in range(npol)] for _ in range(nin)])       # independent periods
    reps = -(-ndat // plan.nsamp_fft)
    rows = np.tile(per, (1, 1, reps))[:, :, :ndat * ndim]
    b = types.SimpleNamespace(case=c, plan=plan, obs=obs, raw=None, scale=1.0, kernel=None, matrix8=None)
    if form == "float":
        b.rows = np.ascontiguousarray(rows.astype(np.float32))
    else:
        # counts c with (c + 0.5) on the scaled period: the unpacker's half step does not pile up in bin 0
        counts = np.clip(np.rint(rows * RMS8 - 0.5), -128, 127).astype(np.int8)
        if form == "caspsr":
            b.raw = np.ascontiguousarray(counts.reshape(2, -1, 4).transpose(1, 0, 2)).ravel()
        else:
            b.raw = np.ascontiguousarray(counts.reshape(nin, npol, ndat, ndim).transpose(2, 0, 1, 3)).ravel()
        b.scale = float(o.S8)
        b.rows = o.unpack_8bit(b.raw, obs, b.scale)
        assert b.rows.shape == rows.shape
    N = plan.n_fft
    krng = np.random.default_rng(_seed(name, 1))
    chirp = np.exp(1j * krng.uniform(-np.pi, np.pi, nin * N)).astype(np.complex64)        # test_gpu_parity._fb_block's, bin 0 KEPT
    if c["matrix"]:
        b.matrix8 = matrix_cases.pack8(matrix_cases.jones_matrices(N, _seed(name, 2) % 1000) * chirp.astype(np.complex128)[:, None, None])
    elif c["kernel"]:
        b.kernel = chirp
    return b


def reference(o, b, dtype, kernel="same"):
    """the oracle's output complex [nchan][npol][npart * nkeep] in `dtype`; kernel: another scalar response (the sensitivity runs)"""
    c, plan = b.case, b.plan
    k = b.kernel if isinstance(kernel, str) else kernel
    if c["matrix"]:
        return matrix_cases.filterbank_matrix(b.rows, plan, b.matrix8, c["npart"], dtype=dtype)
    if c["C"] == 1 and k is not None:
        return o.convolution(b.rows, c["M"], c["nfilt"][0], c["nfilt"][1], k, c["real"], npart=c["npart"], dtype=dtype)
    return o.filterbank(b.rows, plan, k, npart=c["npart"], dtype=dtype)


# ---- the measure -----------------------------------------------------------------------------------------------------------------------
def windows(c):
    """first samples of the M-sample windows: every part boundary where one fits, and the last M samples where those leave a tail"""
    M, nkeep, npart = c["M"], c["M"] - sum(c["nfilt"]), c["npart"]
    total = npart * nkeep
    starts = [p * nkeep for p in range(npart) if p * nkeep + M <= total]
    assert starts, "no window fits"
    if starts[-1] + M < total:
        starts.append(total - M)
    cover = np.zeros(total, bool)
    for s in starts:
        cover[s:s + M] = True
    assert cover.all()
    return starts


def gains(y, c):
    """complex128 [window][nchan][npol][M]: the DFT / M of every window of the output y [nchan][npol][npart * nkeep]"""
    y = np.asarray(y)
    M = c["M"]
    return np.stack([np.fft.fft(y[:, :, s:s + M].astype(np.complex128), axis=-1) / M for s in windows(c)])


def analytic_gains(b, response=True):
    """X[k] kernel[k] exp(2 pi i m (t0 + nfilt_pos) / M) from the transform of ONE period, in float64 (response=False: X[k] alone)"""
    c, plan = b.case, b.plan
    C, M, N = c["C"], c["M"], plan.n_fft
    ndim = 1 if c["real"] else 2
    x = b.rows[:, :, :plan.nsamp_fft * ndim].astype(np.float64)
    X = np.fft.rfft(x, axis=-1)[:, :, :N] if c["real"] else np.fft.fft(np.ascontiguousarray(x).view(np.complex128), axis=-1)
    if not response:
        pass
    elif c["matrix"]:
        d1, d2 = matrix_cases.operate_matrix(X[0, 0], X[0, 1], b.matrix8.astype(np.float64))
        X = np.stack([d1, d2])[None]
    elif b.kernel is not None:
        X = X * b.kernel.astype(np.complex128).reshape(c["input_nchan"], 1, N)
    S = X.reshape(c["input_nchan"], c["npol"], C, M).transpose(0, 2, 1, 3).reshape(c["input_nchan"] * C, c["npol"], M)
    m = np.arange(M)
    return np.stack([S * np.exp(2j * np.pi * ((m * (t0 + c["nfilt"][0])) % M) / M) for t0 in windows(c)])


def figures(G, T):
    """per-bin error of the gains G against the truth T, relative to the rms amplitude of T: rms, worst bin (and where: window, channel,
    polarisation, bin), worst bin 0 of any channel and polarisation"""
    err = np.abs(np.asarray(G) - T)
    amp = math.sqrt(np.mean(np.abs(T) ** 2))
    where = tuple(int(i) for i in np.unravel_index(int(np.argmax(err)), err.shape))
    return dict(rms=math.sqrt(np.mean(err ** 2)) / amp, worst=float(err.max()) / amp, where=where, bin0=float(err[..., 0].max()) / amp,
                amp=amp, err=err)


def structure(err):
    """the error rms of every bin index m over all channels, and of every channel over its bins, each over the rms of all: (largest
    by m, its m, largest by channel, its channel, samples per m, samples per channel).  Evenly spread rounding noise gives values near 1;
    a defect confined to one bin index (the irregular bins 0, M / 2, a table seam) or to some channels stands out."""
    e2 = np.asarray(err) ** 2
    mean = e2.mean()
    by_m = np.sqrt(e2.mean(axis=(0, 1, 2)) / mean)
    by_s = np.sqrt(e2.mean(axis=(0, 2, 3)) / mean)
    return (float(by_m.max()), int(by_m.argmax()), float(by_s.max()), int(by_s.argmax()), e2.size // e2.shape[3], e2.size // e2.shape[1])


def old_measures(got, ref):
    """test_gpu_parity._fb_case's two: rms(err) / rms(ref) and max |err| / rms(ref), and its tolerance for L = 2 C M"""
    err = np.asarray(got).astype(np.complex128) - ref
    rms_ref = math.sqrt(np.mean(np.abs(ref) ** 2))
    return math.sqrt(np.mean(np.abs(err) ** 2)) / rms_ref, float(np.abs(err).max()) / rms_ref


def fb_tolerance(c):
    return 2e-6 * math.sqrt(math.log2(2 * c["C"] * c["M"]))


@functools.lru_cache(maxsize=2)
def truth(name):
    """(the block, the truth's gains, the float32 oracle's figures without the error array -- what the GPU test is judged against -- with
    `periodic`, the largest |y[t + M] - y[t]| of the truth over its maximum, and the truth's shape)"""
    import oracle.dspsr_oracle as o
    b = block(o, by_name(name))
    y = reference(o, b, np.float64)
    M = b.case["M"]
    periodic = float(np.abs(y[:, :, M:] - y[:, :, :-M]).max() / np.abs(y).max()) if y.shape[2] > M else 0.0
    T = gains(y, b.case)
    shape = y.shape
    del y
    f32 = figures(gains(reference(o, b, np.float32), b.case), T)
    del f32["err"]
    f32.update(periodic=periodic, shape=shape)
    return b, T, f32
