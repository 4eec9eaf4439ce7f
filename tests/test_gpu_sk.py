"""dsp::SpectralKurtosis on the device (csrc/sk.hip) against the loop restatement (tests/sk_reference.py).

Exact data (tests/sk_cases.py: small integers, every sum exact in float32 in any order): estimates, tscr estimates, zapmask, cleaned
rows and every counter bit for bit.  Random float rows: the estimates within the bound that follows from the kernel's reduction tree,
then the mask equal to the restated detection of the device's own estimates."""
import numpy as np
import pytest

import dspsr_amd
import sk_reference as ref
from sk_cases import IDS, NOISE, case, chain_length, detector, exact_rows, limits_of, noise_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _place(rows, offset, pad, fill=True):
    """The rows inside a NaN-filled buffer with one spare polarisation row, `pad` + 4 spare floats per row, `offset` floats behind a
    16-byte boundary.  offset 0 with pad a multiple of 4: rows and strides 16-byte aligned; otherwise 8-byte aligned only."""
    import torch
    nchan, npol, n = rows.shape
    row = n + pad + 4
    if offset == 0 and pad % 4 == 0:
        row += -row % 4
    buf = torch.full((nchan, npol + 1, row), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :npol, offset:offset + n]
    if fill:
        view.copy_(torch.from_numpy(rows))
    assert view.data_ptr() % 16 == 4 * offset
    return buf, view


def _engine(ctx, c):
    eng = dspsr_amd.SpectralKurtosisEngine(ctx)
    eng.set_shape(c["nchan"], c["npol"], c["M"])
    eng.set_options(c["std_devs"], c["chans"][0], c["chans"][1], *c["flags"])
    return eng


def _same_statistics(got, want):
    for k in ("zap_counts", "npart_total", "unfiltered_hits", "filtered_hits"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (k, got[k], want[k])
    for k in ("filtered_sum", "unfiltered_sum"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k


@pytest.mark.parametrize("name", IDS)
def test_exact_rows_bit_for_bit(ctx, name):
    import torch
    c = case(name)
    M, nchan, npol, npart, ndat = c["M"], c["nchan"], c["npol"], c["npart"], c["ndat"]
    rows = exact_rows(c)
    est, est_tscr = ref.compute(rows, M, c["flags"][1])
    limits, limits_tscr = limits_of(c)
    det = detector(c)
    mask = det.detect(est, est_tscr, limits, limits_tscr).copy()
    clean = ref.mask_rows(rows, mask, M)

    eng = _engine(ctx, c)
    buf, view = _place(rows, c["offset"], c["pad"])
    before = buf.cpu().numpy()
    # out of place, into rows placed another way: behind the npart * M samples nothing is written
    obuf, oview = _place(rows, 2 - c["offset"], c["pad"] + 2, fill=False)
    assert eng.transform(view, oview, ndat) == npart * M and eng.npart == npart
    assert np.array_equal(_bits(eng.estimates()), _bits(est))
    if not c["flags"][1]:
        assert np.array_equal(_bits(eng.estimates_tscr()), _bits(est_tscr))
    assert np.array_equal(eng.zapmask(), mask)
    want = np.full(tuple(obuf.shape), np.nan, np.float32)
    want[:, :npol, 2 - c["offset"]:2 - c["offset"] + 2 * npart * M] = clean
    assert np.array_equal(_bits(obuf.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(before))             # the input is only read
    _same_statistics(eng.get_statistics(), det.statistics())

    # in place: the same rows, and the counters go on from the first call (float sums in part order)
    assert eng.transform(view, view, ndat) == npart * M
    want = before.copy()
    want[:, :npol, c["offset"]:c["offset"] + 2 * npart * M] = clean
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(want))
    assert np.array_equal(eng.zapmask(), mask)
    det.detect(est, est_tscr, limits, limits_tscr)
    _same_statistics(eng.get_statistics(), det.statistics())
    eng.reset_count()
    stats = eng.get_statistics()
    assert not stats["zap_counts"].any() and stats["npart_total"] == 0 and not stats["filtered_sum"].any()

    # a stream cut into calls of 1, 3 and all parts gives the same estimates
    view.copy_(torch.from_numpy(rows))
    for step in (1, 3, npart):
        got = []
        for p0 in range(0, npart, step):
            n = min(step, npart - p0)
            eng.compute(view[:, :, 2 * M * p0:], n * M + (c["rem"] if p0 + n == npart else 0))
            assert eng.npart == n
            got.append(eng.estimates())
        assert np.array_equal(_bits(np.concatenate(got)), _bits(est)), step
    eng.close()


def test_an_estimate_equal_to_a_limit_is_not_zapped(ctx):
    c = case("m128_c64_p2_n64")
    rows = exact_rows(c)
    est, _ = ref.compute(rows, c["M"])
    eng = _engine(ctx, c)
    _, view = _place(rows, 0, 0)
    eng.compute(view, c["ndat"])
    lo, hi = np.float32(0), est.max()
    eng.reset_mask()
    eng.detect_skfb(lo, hi)
    assert not eng.zapmask().any() and eng.get_statistics()["zap_counts"][eng.ZAP_SKFB] == 0
    det = detector(c)
    det.reset_mask(c["npart"])
    lo, hi = np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0))
    det.detect_skfb(est, lo, hi)
    eng.detect_skfb(lo, hi)
    assert det.mask.any() and np.array_equal(eng.zapmask(), det.mask)
    assert eng.get_statistics()["zap_counts"][eng.ZAP_SKFB] == det.zap_counts[ref.ZAP_SKFB]
    eng.close()


@pytest.mark.parametrize("index", range(len(NOISE)), ids=["m%d" % n[0] for n in NOISE])
def test_random_rows_within_the_bound_of_the_tree(ctx, index):
    """k_sk_compute adds the M terms of S1 and of S2 in a tree whose longest chain of additions is L = L(M) = 2 * ceil(ceil(P / W) / 4)
    - 1 + 2 + log2(W), P = ceil(M / 2) pairs dealt to W = 16 (P <= 64), 32 (P <= 128) or 64 lanes (csrc/sk.hip; chain_length restates
    it: L(32) = 7, L(128) = 7, L(1024) = 11, L(65536) = 263).  With u = 2^-24: |x|^2 carries 2 roundings and |x|^4 one more, each term then passes
    through at most L additions, so S1 and S2 each have a relative error <= (L + 4) u to first order (non-negative terms: the relative
    errors do not grow in the sum).  est = M_fac * (M * S2 / S1^2 - 1): S1^2 doubles S1's error and adds a rounding, the quotient, the
    product with M and the difference one each, so M * S2 / S1^2 = (est / M_fac + 1) is off by <= (3 (L + 4) + 3) u relative, and the
    subtraction and the last product add 1 u of the result each:  |d est| <= (3 L + 16) u (est + M_fac).
    The tscr estimate adds the npart values of S1 and S2 in sequence: L + npart in the place of L.
    Detection is exact arithmetic on the estimates: the mask must EQUAL the restated detection run on the device's own estimates."""
    M, nchan, npol, npart, rem = NOISE[index]
    c = dict(M=M, nchan=nchan, npol=npol, npart=npart, std_devs=3, chans=(0, 0), flags=(False, False, False))
    rows = noise_rows(index)
    want, want_tscr = ref.compute(rows, M, dtype=np.float64)
    eng = _engine(ctx, c)
    offset = 0 if index % 2 == 0 else 2
    buf, view = _place(rows, offset, 4 * index)
    eng.transform(view, view, npart * M + rem)
    est, est_tscr, mask = eng.estimates(), eng.estimates_tscr(), eng.zapmask()
    u, L, m_fac = 2.0 ** -24, chain_length(M), (M + 1) // (M - 1)
    err = np.abs(est.astype(np.float64) - want)
    print("M=%d L=%d max |d est| / bound = %.3g" % (M, L, (err / ((3 * L + 16) * u * (want + m_fac))).max()))
    assert (err <= (3 * L + 16) * u * (want + m_fac)).all()
    m_t = float(M * npart)
    err = np.abs(est_tscr.astype(np.float64) - want_tscr)
    assert (err <= (3 * (L + npart) + 16) * u * (want_tscr + (m_t + 1) / (m_t - 1))).all()
    det = detector(c)
    limits, limits_tscr = limits_of(c)
    assert np.array_equal(det.detect(est, est_tscr, limits, limits_tscr), mask)
    _same_statistics(eng.get_statistics(), det.statistics())
    got = buf.cpu().numpy()[:, :npol, offset:offset + rows.shape[2]]
    want_rows = rows.copy()
    want_rows[:, :, :2 * npart * M] = ref.mask_rows(rows, mask, M)
    assert np.array_equal(_bits(got), _bits(want_rows))                        # +0.0 where the mask is set, the input elsewhere
    eng.close()


def test_refusals_by_name(ctx):
    import torch
    eng = dspsr_amd.SpectralKurtosisEngine(ctx)
    x = torch.zeros((2, 2, 2 * 64 + 4), dtype=torch.float32, device="cuda")
    with pytest.raises(dspsr_amd.DspsrAmdError, match="no shape"):
        eng.compute(x, 64)
    for shape, text in (((2, 2, 31), r"M=31 outside \[32, 65536\]"), ((2, 2, 65537), r"M=65537 outside \[32, 65536\]"),
                        ((2, 3, 32), "npol=3 not 1 or 2"), ((0, 2, 32), r"nchan=0 outside \[1, 65535\]"),
                        ((65536, 2, 32), r"nchan=65536 outside \[1, 65535\]")):
        with pytest.raises(dspsr_amd.DspsrAmdError, match=text):
            eng.set_shape(*shape)
    eng.set_shape(2, 2, 32)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="std_devs == 0"):
        eng.set_options(0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="chan_start=1 >= chan_end=1"):
        eng.set_options(3, 1, 1)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="chan_start=2 >= chan_end=2"):
        eng.set_options(3, 2, 0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="chan_end=3 > nchan=2"):
        eng.set_options(3, 0, 3)
    with pytest.raises(dspsr_amd.DspsrAmdError, match=r"ndat=2147483648 >= 2\^31"):
        eng.compute(x, 1 << 31)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="input rows must be 8-byte aligned"):
        eng.compute(x[:, :, 1:], 64)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="input rows must be 8-byte aligned"):
        eng.compute(torch.zeros((2, 2, 2 * 64 + 1), dtype=torch.float32, device="cuda"), 64)      # an odd stride
    with pytest.raises(dspsr_amd.DspsrAmdError, match="input stride shorter than the row of 256 floats"):
        eng.compute(x, 128)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="input rows overlap"):
        eng.compute(torch.as_strided(x, (2, 2, 128), (160, 128, 1)), 64)
    eng.compute(x, 64)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="input and output rows partly overlap"):
        eng.mask(x[:, :, :128], x[:, :, 2:130])
    with pytest.raises(dspsr_amd.DspsrAmdError, match="in place with different strides"):
        eng.mask(x, torch.as_strided(x, (2, 2, 128), (2 * 132 + 2, 132, 1)))
    # fewer samples than one part: nothing to do, no error
    eng.compute(x, 31)
    assert eng.npart == 0 and eng.transform(x, x, 31) == 0 and eng.zapmask().shape == (0, 2)
    assert eng.get_statistics()["npart_total"] == 0
    eng.close()
