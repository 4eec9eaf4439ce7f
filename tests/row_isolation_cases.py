"""Which input each filterbank output depends on (tests/test_gpu_row_isolation.py, tests/test_row_isolation_cases_host.py): the case
table, the perturbations and the masks of what must not change, as plain data and numpy.  No torch.  Inputs, plans, responses, oracles
and the per-bin measure are those of tests/transfer_cases.py; a case of the same name there has the same baseline block here.

The property is the reference's data flow: output (channel c of input channel i, polarisation p, part j) depends on the nsamp_fft
samples of part j of input row (i, p) and on nothing else -- with a matrix response on both polarisations of (i, part j).  Every
accuracy test of the filterbank feeds all rows the same amplitude and divides the error by the rms of the whole output, so an error
confined to one row and proportional to ANOTHER row's amplitude is invisible to them.  Here one target at a time is changed (another
period, 2^-12 of its amplitude, nothing at all, a NaN) and everything the data flow says is unaffected must come back bit for bit.

`rows` of a case: "independent" -- the device keeps the property, all checks are equalities; "paired" -- the two polarisations of
real input enter ONE complex transform, W = X0 + i X1, and come apart in a Hermitian split, so each holds the rounding noise of the
other.  That is by design on the paths below, and the price is measured per row instead (pair_figures)."""
import copy
import math

import numpy as np

import transfer_cases as tc

WEAK_LOG2 = -12                       # float rows: the target scaled by 2^-12 (exact); perform_raw: the scale of the whole block
WEAK_RAW = tc.RMS8 / 8                # 8-bit rows: the target drawn at an eighth of the counts (3 counts per unit of `period`)
KINDS = ("other", "weak", "dead", "poison", "first", "last", "silent", "scale")
ROW_KINDS = ("other", "weak", "dead", "poison")       # one target row (or input channel) changes, over all parts
SEED_OTHER, SEED_EDGE = 7, 8          # transfer_cases._seed(name, k): 0 the baseline's periods, 1 the response, 2 the Jones matrices

# Where the polarisations of real dual-polarisation input share one transform (dspsr_amd/csrc):
#   fb_inv_chan.h:310-318       k_inv_chan, the split in the inverse pass (split_in_inverse, the sub-band and odd-factor paths)
#   fb_inv_chan.h:299-306       the same ahead of a matrix response
#   fb_fwd_rows.hip:181-183, 205-207   k_fwd_rows_split, the pre-split default: the split at the end of pass 2
#   fb_four_pass.hip:222-225    k_inv_a, the four-pass form
# All of them undo the pairing pass 1 makes for every real dual-polarisation call on these paths (the loaders of fb_fwd_cols.hip take one
# element = (pol0, pol1) of a real sample); fb_plain.hip transforms one polarisation per tile and pairs nothing.
PAIRED_SITE = "real input, two polarisations: W = X0 + i X1 through passes 1 and 2, Hermitian split at %s"


def _case(site, rows, *a, where=None, **kw):
    c = dict(tc.make_case(*a, **kw))
    assert rows in ("independent", "paired")
    assert (rows == "paired") == (where is not None), site
    c.update(site=site, rows=rows, where=PAIRED_SITE % where if where else None)
    return c


def _cases():
    P, I = "paired", "independent"
    split2, split3 = "fb_fwd_rows.hip:181-183/205-207", "fb_inv_chan.h:310-318"
    odd_c = (24, 256)                                    # three sub-bands of 8 channels: L = 12288, several tiles per pass
    out = [
        # ---- real input, two polarisations, on tiles
        _case("real2 pre-split", P, "three", 16, 256, True, where=split2),
        _case("real2 split in inverse", P, "three", 16, 256, True, sii=True, where=split3),
        _case("real2 four passes forced", P, "four", 16, 256, True, four=1, where="fb_four_pass.hip:222-225"),
        _case("real2 caspsr", P, "three", 16, 256, True, form="caspsr", where=split2),
        _case("real2 float rows", P, "three", 16, 256, True, form="float", where=split2),
        _case("real2 full tile", P, "three", 4, 4096, True, where=split2),
        _case("real2 four passes by length", P, "four", 2, 16384, True, where="fb_four_pass.hip:222-225"),
        _case("real2 odd_C", P, "odd_C", *odd_c, True, where=split3),
        _case("real2 odd_M", P, "odd_M", 16, 640, True, where=split3),
        _case("real2 subbands", P, "subbands", 16, 256, True, input_nchan=2, where=split2 + " or " + split3),
        _case("real2 matrix pre-split", P, "matrix", 16, 256, True, matrix=True, where=split2),
        _case("real2 matrix split in inverse", P, "matrix", 16, 256, True, matrix=True, sii=True, where="fb_inv_chan.h:299-306"),
        # ---- real input, one polarisation: W = X0 + i 0, the split's second output is dropped
        _case("real1", I, "three", 16, 256, True, npol=1),
        # ---- complex input
        _case("complex2", I, "three", 32, 128, False),
        _case("complex1", I, "three", 32, 128, False, npol=1),
        _case("complex2 four passes forced", I, "four", 32, 128, False, four=1),         # fb_four_pass.hip:227, `npol2 ? q.b : 0`
        _case("complex1 four passes forced", I, "four", 32, 128, False, npol=1, four=1),
        _case("complex2 two passes", I, "two", 16, 512, False),
        _case("complex2 subbands float", I, "subbands", 32, 128, False, input_nchan=4, form="float"),
        _case("complex2 batched", I, "batched", 1, 1024, False, form="float", input_nchan=4, four=1),
        _case("complex2 matrix", I, "matrix", 32, 128, False, matrix=True),
        _case("conv1 short", I, "conv1", 1, 64, False, form="float", input_nchan=3),
        _case("conv1 long", I, "conv1", 1, 4096, False, form="float", input_nchan=3),
        _case("conv3", I, "conv3", 1, 16384, False, form="float", input_nchan=3),
        # ---- freq_res 1
        _case("plain raw8", I, "plain", 64, 1, True, npart=70),
        _case("plain float", I, "plain", 64, 1, True, form="float", npart=70),
        # ---- no response at all, one per family
        _case("nokernel three", P, "three", 16, 256, True, kernel=False, where=split2),
        _case("nokernel two", I, "two", 16, 512, False, kernel=False),
        _case("nokernel odd_C", P, "odd_C", *odd_c, True, kernel=False, where=split3),
        _case("nokernel subbands", P, "subbands", 16, 256, True, input_nchan=2, kernel=False, where=split2 + " or " + split3),
        _case("nokernel plain", I, "plain", 64, 1, True, npart=70, kernel=False),
        _case("nokernel conv1", I, "conv1", 1, 4096, False, form="float", input_nchan=3, kernel=False),
        _case("nokernel batched", I, "batched", 1, 1024, False, form="float", input_nchan=4, four=1, kernel=False),
    ]
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]
SITES = [c["site"] for c in CASES]


def by_name(name):
    return CASES[NAMES.index(name)]


def is_float(c):
    return c["form"] == "float"


def pairs_by_construction(c):
    """what the code read says: real input with two polarisations on the tile, odd and sub-band paths"""
    return c["real"] and c["npol"] == 2 and c["picks"]["path"] in ("tiles", "odd")


def targets(c):
    """polarisation 1 and polarisation 0 of input channel 0 and, where there are several, one whole input channel"""
    t = [("pol", p) for p in range(c["npol"] - 1, -1, -1)]
    if c["input_nchan"] > 1:
        t.append(("chan", c["input_nchan"] // 2))
    return t


def target_rows(c, target):
    """the input rows (input channel, polarisation) of a target"""
    what, k = target
    return [(0, k)] if what == "pol" else [(k, p) for p in range(c["npol"])]


def alone(c):
    """one input channel whose rows all depend on the target: one polarisation, or two behind a matrix response"""
    return c["input_nchan"] == 1 and (c["npol"] == 1 or c["matrix"])


def runs(c):
    """every (kind, target) of a case that has something to assert.  poison: float rows only (8 bits hold no NaN); scale: perform_raw
    only; silent on 8-bit rows only where some part does not overlap part 1 (freq_res 1) -- its zeros are a float property; where
    no row is left that the target does not reach (`alone`), other / weak / dead only if the pair is measured or the row is float."""
    out = []
    for kind in KINDS:
        if kind in ROW_KINDS:
            if kind == "poison" and not is_float(c):
                continue
            if kind != "poison" and alone(c) and c["rows"] != "paired" and (c["matrix"] or not is_float(c) or kind == "other"):
                continue
            out += [(kind, t) for t in targets(c)]
        elif kind == "scale":
            if not is_float(c):
                out.append((kind, None))
        elif kind == "silent":
            if is_float(c) or c["M"] == 1:
                out.append((kind, None))
        else:
            out.append((kind, None))
    return out


# ---- blocks ----------------------------------------------------------------------------------------------------------------------------
def _periods(c, plan, k):
    rng = np.random.default_rng(tc._seed(c["name"], k))
    return np.stack([[tc.period(plan.nsamp_fft, c["real"], rng) for _ in range(c["npol"])] for _ in range(c["input_nchan"])])


def _tiled(per, ndat, ndim):
    reps = -(-ndat * ndim // per.shape[2])
    return np.tile(per, (1, 1, reps))[:, :, :ndat * ndim]


def _counts(rows, amp=tc.RMS8):
    return np.clip(np.rint(rows * amp - 0.5), -128, 127).astype(np.int8)            # transfer_cases.block's


def _layout(counts, c):
    """int8 [input_nchan][npol][ndat * ndim] in the order of the case's 8-bit block"""
    nin, npol = counts.shape[:2]
    if c["form"] == "caspsr":
        return np.ascontiguousarray(counts.reshape(2, -1, 4).transpose(1, 0, 2)).ravel()
    ndim = 1 if c["real"] else 2
    return np.ascontiguousarray(counts.reshape(nin, npol, -1, ndim).transpose(2, 0, 1, 3)).ravel()


def baseline(o, c):
    """transfer_cases.block with what the perturbations need beside it: ndat and, for 8-bit forms, the counts row by row"""
    b = tc.block(o, c)
    ndim = b.obs.ndim
    b.ndat = b.rows.shape[2] // ndim
    b.counts = None
    if b.raw is not None:
        b.counts = _counts(_tiled(_periods(c, b.plan, 0), b.ndat, ndim))
        assert np.array_equal(_layout(b.counts, c), b.raw)
    return b


def poison_sample(b):
    """the sample that turns NaN: the middle of part 1's window"""
    return b.plan.nsamp_step + b.plan.nsamp_fft // 2


def perturbed(o, b, kind, target=None):
    """The block with one perturbation; every other float or byte as in the baseline b (which is left as it is)."""
    c, plan = b.case, b.plan
    ndim, step, fft = b.obs.ndim, plan.nsamp_step, plan.nsamp_fft
    p = copy.copy(b)
    if kind == "scale":
        assert b.raw is not None
        p.scale = math.ldexp(b.scale, WEAK_LOG2)
        p.rows = o.unpack_8bit(b.raw, b.obs, p.scale)
        return p
    flt = b.raw is None
    data = (b.rows if flt else b.counts).copy()

    def fresh(k, amp=tc.RMS8):
        rows = _tiled(_periods(c, plan, k), b.ndat, ndim)
        return rows.astype(np.float32) if flt else _counts(rows, amp)
    if kind in ROW_KINDS:
        for i, pol in target_rows(c, target):
            if kind == "other":
                data[i, pol] = fresh(SEED_OTHER)[i, pol]
            elif kind == "weak":
                data[i, pol] = np.ldexp(data[i, pol], WEAK_LOG2) if flt else fresh(0, WEAK_RAW)[i, pol]
            elif kind == "dead":
                data[i, pol] = 0
            else:
                assert flt, "8 bits hold no NaN"
                data[i, pol, poison_sample(b) * ndim] = np.nan
    elif kind == "first":
        data[:, :, :step * ndim] = fresh(SEED_EDGE)[:, :, :step * ndim]
    elif kind == "last":
        data[:, :, (b.ndat - step) * ndim:] = fresh(SEED_EDGE)[:, :, (b.ndat - step) * ndim:]
    elif kind == "silent":
        data[:, :, step * ndim:(step + fft) * ndim] = 0
    else:
        raise ValueError(kind)
    if flt:
        p.rows = data
    else:
        p.counts = data
        p.raw = _layout(data, c)
        p.rows = o.unpack_8bit(p.raw, b.obs, b.scale)
        assert p.rows.shape == b.rows.shape
    return p


# ---- what depends on what --------------------------------------------------------------------------------------------------------------
def parts_reading(b, lo, hi):
    """the parts whose nsamp_fft input samples meet the samples [lo, hi)"""
    step, fft = b.plan.nsamp_step, b.plan.nsamp_fft
    return [j for j in range(b.case["npart"]) if j * step < hi and lo < j * step + fft]


def touched_parts(b, kind):
    step, fft = b.plan.nsamp_step, b.plan.nsamp_fft
    if kind == "first":
        return parts_reading(b, 0, step)
    if kind == "last":
        return parts_reading(b, b.ndat - step, b.ndat)
    if kind == "silent":
        return parts_reading(b, step, step + fft)
    if kind == "poison":
        return parts_reading(b, poison_sample(b), poison_sample(b) + 1)
    return list(range(b.case["npart"]))


def expand(b, row_mask, parts):
    """bool [nchan][npol][npart * nkeep] from bool [input_nchan][npol] and a list of parts"""
    c, nkeep = b.case, b.plan.nkeep
    pm = np.zeros(c["npart"], bool)
    pm[list(parts)] = True
    rows = np.repeat(row_mask, c["C"], axis=0)
    return rows[:, :, None] & np.repeat(pm, nkeep)[None, None, :]


def target_mask(b, target):
    """bool [input_nchan][npol]: the rows of the target (None: all rows)"""
    c = b.case
    m = np.zeros((c["input_nchan"], c["npol"]), bool)
    if target is None:
        m[:] = True
    else:
        for i, pol in target_rows(c, target):
            m[i, pol] = True
    return m


def may_change(b, kind, target, paired):
    """bool [nchan][npol][npart * nkeep]: the outputs that depend on what the perturbation changed.  paired: the polarisations of an
    input channel count as one (the device's paired paths; a matrix response always)."""
    if kind == "scale":
        return expand(b, target_mask(b, None), range(b.case["npart"]))
    rows = target_mask(b, target)
    if paired or b.case["matrix"]:
        rows = rows | rows.any(axis=1, keepdims=True)
    return expand(b, rows, touched_parts(b, kind))


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view(np.int32 if y.dtype == np.complex64 else np.int64)


def is_zero(y):
    """every float +0 or -0"""
    v = bits(y)
    return (v & np.iinfo(v.dtype).max) == 0


def check_equalities(b, base, got, kind, target, paired):
    """Every equality of a run, for the oracles (paired False: the reference pairs nothing) and the device alike.  base, got: complex
    [nchan][npol][npart * nkeep] of the baseline and of the perturbed block.  Returns the number of floats compared; raises
    AssertionError naming the first output that differs."""
    c = b.case
    flt = is_float(c)
    shape = base.shape
    two = (shape[0], shape[1], shape[2], 2)
    vb, vg = bits(base).reshape(two), bits(got).reshape(two)

    def first(bad):
        ch, pol, t, _ = (int(i) for i in np.unravel_index(int(np.argmax(bad)), bad.shape))
        return "channel %d (input channel %d) polarisation %d part %d sample %d" % (ch, ch // c["C"], pol, t // b.plan.nkeep, t % b.plan.nkeep)
    nfloat = 0
    if kind == "scale":
        want = bits(np.ldexp(base.view(base.real.dtype), WEAK_LOG2).view(base.dtype)).reshape(two)
        bad = want != vg
        assert not bad.any(), "%s scale x 2^%d: %d floats are not the baseline's x 2^%d, first %s" % (
            c["name"], WEAK_LOG2, bad.sum(), WEAK_LOG2, first(bad))
        return want.size
    # locality
    same = ~may_change(b, kind, target, paired)
    bad = (vb != vg) & same[..., None]
    assert not bad.any(), "%s %s %s: %d floats that do not depend on it changed, first %s" % (c["name"], kind, target, bad.sum(), first(bad))
    nfloat += 2 * int(same.sum())
    tm = target_mask(b, target)
    independent = not (paired or c["matrix"])
    if flt and kind == "weak" and independent:
        m = expand(b, tm, range(c["npart"]))
        want = bits(np.ldexp(base.view(base.real.dtype), WEAK_LOG2).view(base.dtype)).reshape(two)
        bad = (want != vg) & m[..., None]
        assert not bad.any(), "%s weak %s: %d floats of the target are not the baseline's x 2^%d, first %s" % (
            c["name"], target, bad.sum(), WEAK_LOG2, first(bad))
        nfloat += 2 * int(m.sum())
    if flt and kind == "dead" and independent:
        m = expand(b, tm, range(c["npart"]))
        bad = ~is_zero(got).reshape(two) & m[..., None]
        assert not bad.any(), "%s dead %s: %d floats of the target are not zero, first %s" % (c["name"], target, bad.sum(), first(bad))
        nfloat += 2 * int(m.sum())
    if flt and kind == "silent":
        m = expand(b, target_mask(b, None), [1])
        bad = ~is_zero(got).reshape(two) & m[..., None]
        assert not bad.any(), "%s silent: %d floats of part 1 are not zero, first %s" % (c["name"], bad.sum(), first(bad))
        nfloat += 2 * int(m.sum())
    if kind == "poison":
        # every output channel of the target row holds a NaN in every part that reads the sample
        nkeep = b.plan.nkeep
        nan = np.isnan(got.real) | np.isnan(got.imag)
        for j in touched_parts(b, kind):
            per_row = nan[:, :, j * nkeep:(j + 1) * nkeep].any(axis=2)
            missing = np.repeat(tm, c["C"], axis=0) & ~per_row
            assert not missing.any(), "%s poison %s: part %d of %d output rows holds no NaN" % (c["name"], target, j, missing.sum())
        nfloat += 1
    return nfloat


def partner_unchanged(b, base, got, target):
    """True where the other polarisation of a polarisation target came back bit for bit: the rows are not paired after all"""
    i, pol = target_rows(b.case, target)[0]
    m = np.zeros((b.case["input_nchan"], b.case["npol"]), bool)
    m[i, 1 - pol] = True
    m = expand(b, m, range(b.case["npart"]))
    return bool((bits(base).reshape(m.shape + (2,)) == bits(got).reshape(m.shape + (2,)))[m].all())


# ---- the price of a pair ---------------------------------------------------------------------------------------------------------------
def pair_figures(G, T, c, i):
    """Per row of input channel i (its C output channels, polarisation p): the per-bin error of the gains G against the truth T
    [window][nchan][npol][M] relative to the rms amplitude OF THE PAIR -- sqrt of the mean of the two rows' mean squares -- as rms and
    worst bin, the same two over both rows, the row's own rms amplitude and the error array of each row."""
    sl = slice(i * c["C"], (i + 1) * c["C"])
    err = np.abs(np.asarray(G)[:, sl] - T[:, sl])
    a2 = (np.abs(T[:, sl]) ** 2).mean(axis=(0, 1, 3))                                # mean square of each row
    amp = math.sqrt(a2.mean())
    rows = []
    for p in range(c["npol"]):
        e = err[:, :, p:p + 1, :]
        rows.append(dict(rms=math.sqrt(np.mean(e ** 2)) / amp, worst=float(e.max()) / amp, own=math.sqrt(a2[p]), err=e))
    return dict(amp=amp, rms=math.sqrt(np.mean(err ** 2)) / amp, worst=float(err.max()) / amp, rows=rows)
