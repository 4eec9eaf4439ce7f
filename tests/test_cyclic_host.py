"""Cyclic-spectrum folding, the parts that need no device: the two bin plans, Synch (window + backward complex-to-real
transform) and the restatement itself against the mathematics of a gated tone."""
import numpy as np
import pytest

import cyclic_reference as cr
import dspsr_amd


def test_case_table_is_exact():
    for case in cr.EXACT_CASES:
        cr.check_exact(case)
    assert {c["nlag"] for c in cr.EXACT_CASES} == {2, 3, 33, 129, 513, 2049}
    assert {(c["npol_in"], c["npol_out"]) for c in cr.EXACT_CASES} == {(1, 1), (2, 1), (2, 2), (2, 4)}
    assert min(c["nbin"] for c in cr.EXACT_CASES) == 2 and max(c["nbin"] for c in cr.EXACT_CASES) == 1024


def test_binplan_equals_the_restatement():
    rng = np.random.default_rng(7)
    for trial in range(40):
        nbin = int(rng.choice([1, 2, 3, 7, 64, 1000, 1024, 4096]))
        phi = float(rng.uniform(-5, 5)) if trial % 2 else float(rng.uniform(0, 1))
        # steps from a thousandth of a bin to several bins per sample
        pps = float(10 ** rng.uniform(-3, 0.8) / nbin)
        ndat = int(rng.integers(1, 3000))
        p0, p1, hits = dspsr_amd.cyclic_binplan(phi, pps, nbin, ndat)
        r0, r1, rhits = cr.plans(phi, pps, nbin, ndat)
        assert np.array_equal(p0, r0) and np.array_equal(p1, r1) and np.array_equal(hits, rhits), (nbin, phi, pps, ndat)
        assert hits.sum() == ndat
        plan, fhits = dspsr_amd.fold_binplan(phi, pps, nbin, ndat)      # plan0 is the fold plan itself
        assert np.array_equal(plan, p0) and np.array_equal(fhits, hits)


def _positive_lags(rng, nbin, npol, nchan, nlag):
    """lag functions of positive spectra (what a fold of voltages gives): rfft of a positive row / n"""
    n = 2 * nlag - 2
    spec = rng.uniform(0.5, 1.5, size=(nbin, npol, nchan, n))
    lags = np.fft.rfft(spec, axis=3) / n
    # the two real-valued ends carry an imaginary part in the fold's output that the transform must ignore
    lags[..., 0] += 0.25j
    lags[..., -1] -= 0.5j
    return lags.astype(np.complex64)


@pytest.mark.parametrize("nlag,mover", [(2, 1), (2, 2), (3, 1), (3, 2), (3, 4), (33, 1), (33, 2), (33, 4), (2049, 1), (2049, 2),
                                        (2049, 4)])
def test_lags_to_spectra_against_irfft(nlag, mover):
    rng = np.random.default_rng(nlag * 8 + mover)
    nbin, npol, nchan = 3, 2, 2
    lags = _positive_lags(rng, nbin, npol, nchan, nlag)
    got = dspsr_amd.cyclic_lags_to_spectra(np.stack([lags.real, lags.imag], axis=-1), mover)
    ref = cr.synch(lags, mover)
    n = 2 * nlag - 2
    assert got.shape == ref.shape == (nchan * n // mover, npol, nbin) and got.dtype == np.float32
    # Tolerance.  A radix-2 transform of n points takes every output through log2(n) butterflies; each is one rounded complex
    # multiplication by a float twiddle and one rounded addition, so a value picks up at most two float32 roundings (2 * 2^-24
    # of its magnitude) per stage, and magnitudes inside the transform of a positive spectrum never exceed the largest output
    # (the partial sums of non-negative terms).  One more stage's worth covers the window product and the rounded twiddles.
    # Relative to the row's largest value: (log2(n) + 1) * 2^-23.
    tol = (np.log2(n) + 1) * 2.0 ** -23
    per = n // mover
    g = got.reshape(nchan, per, npol, nbin).astype(np.float64)
    r = ref.reshape(nchan, per, npol, nbin)
    err = np.abs(g - r).max(axis=1) / np.abs(r).max(axis=1)
    assert err.max() <= tol, "nlag %d mover %d: error %.3g of the row's largest value > %.3g" % (nlag, mover, err.max(), tol)


def test_lags_to_spectra_refuses_other_lengths():
    lags = np.zeros((2, 1, 1, 4, 2), np.float32)                        # nchan_spec = 6
    with pytest.raises(dspsr_amd.DspsrAmdError):
        dspsr_amd.cyclic_lags_to_spectra(lags, 1)


def test_float32_restatement_is_exact_on_integer_rows():
    """on the exact data the float32 strict-order sums and the float64 sums are the same integers"""
    case = cr.EXACT_CASES[1]
    for (rows, _, lags32), (ndat, start, phi, pps, _) in zip(cr.exact_reference(1)[:1], case["calls"][:1]):
        p0, p1, _ = cr.plans(phi, pps, case["nbin"], ndat)
        l64 = cr.fold(rows[:, :, start:], p0, p1, case["nlag"], case["npol_out"], case["nbin"])
        assert np.array_equal(l64.astype(np.complex64), lags32)
    steps = cr.exact_reference(0)
    assert not steps[0][2].any(), "ndat_fold = nlag must accumulate nothing"
    assert steps[1][2].any(), "ndat_fold = nlag + 1 folds one sample"


@pytest.mark.parametrize("k", [5, 23, 40])
def test_gated_tone_lands_in_its_cyclic_channel(k):
    """Physical anchor.  x[t] = g(t) exp(2 pi i k t / n), n = nchan_spec = 2 nlag - 2, g = 1 inside a phase window and 0 outside.
    Then x[t] conj(x[t + l]) = g(t) g(t + l) exp(-2 pi i k l / n): the lag function of every bin is c_l exp(-2 pi i k l / n) with
    c_l >= 0, and the backward transform sum_l z_l exp(+2 pi i j l / n) is largest where j = k -- output channel k itself, not
    the mirrored n - k (k = 40 > n / 2 is a negative frequency and still lands in channel 40).  A product needs both samples
    inside the window, and its bin is that of the midpoint t + l / 2, which then lies inside the window too: bins outside
    the gate receive exactly nothing."""
    nlag, nbin, ndat = 33, 16, 6000
    n = 2 * nlag - 2
    period = 800.0                                                       # samples: 50 per bin, a gate of 4 bins = 200 > nlag
    pps = 1.0 / period
    p0, p1, _ = cr.plans(0.0, pps, nbin, ndat)
    t = np.arange(ndat)
    gate_bins = [5, 6, 7, 8]
    g = np.isin(p0, gate_bins).astype(np.float64)                        # the window in the plan's own phases
    x = (g * np.exp(2j * np.pi * k * t / n))[None, None, :]
    lags = cr.fold(x, p0, p1, nlag, 1, nbin)
    spec = cr.synch(lags, 1)[:, 0, :]                                    # [channel][bin]
    off = [b for b in range(nbin) if b not in gate_bins]
    assert not spec[:, off].any(), "power outside the gated bins"
    for b in gate_bins[1:-1]:                                            # bins wholly inside the gate
        assert spec[:, b].argmax() == k
        assert spec[k, b] > 10 * np.abs(np.delete(spec[:, b], [k - 1, k, (k + 1) % n])).max()
