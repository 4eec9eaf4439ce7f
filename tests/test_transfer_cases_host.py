"""tests/transfer_cases.py without a GPU: the periodic-input measurement on the oracle alone (the truth is M-periodic, equals the
analytic gain and has no weak bin; a response bin changed by 1e-5 is found at that bin, at that size, while both measures of
test_gpu_parity._fb_case stay inside their bounds), the float32 baseline every case of tests/test_gpu_transfer.py is judged against,
and the coverage of the table: the restated kernel picks of its cases are exactly the set a call with L <= 2^22 reaches, and every
instantiation outside that set stands in transfer_cases.PINNED with its reason."""
import math

import numpy as np
import pytest

import fused_fold_cases as ffc
import transfer_cases as tc


def test_table_size_and_names():
    assert len(set(tc.NAMES)) == len(tc.NAMES)
    assert 250 <= len(tc.CASES) <= 400
    for c in tc.CASES:
        assert c["picks"]["path"] in tc.EXPECTED_PATH[c["family"]], c["name"]
        nkeep = c["M"] - sum(c["nfilt"])
        assert 2 * nkeep >= c["M"] and c["max_parts"] >= 2 and c["npart"] > 2, c["name"]
        assert c["M"] == 1 or c["nfilt"][0] >= 1, c["name"]
        assert c["picks"]["L"] <= 1 << tc.MAX_LOG_L and c["M"] <= 1 << tc.MAX_LOG_FRES


def test_picks_agree_with_the_fused_fold_restatement():
    """fused_fold_cases.geometry restates fb_tile for dual-polarisation objects: the same passes and the same inverse tile"""
    for c in tc.CASES:
        if c["family"] not in ("three", "four", "two") or c["npol"] != 2 or c["input_nchan"] != 1 or c["C"] < 2:
            continue
        g = ffc.geometry(c["C"], c["M"], c["nfilt"], c["real"], force_four_pass=c["four"], raw8=c["form"] == "raw8")
        assert g["passes"] == c["picks"]["passes"], c["name"]
        p3 = [t for t in c["picks"]["tuples"] if t[0] == "p3"]
        if p3:
            assert p3[0][2] == (g["logT3"] + 1 == 14 - g["logM"]), c["name"]


def test_coverage_is_the_reachable_set_and_the_rest_is_pinned():
    reach, inst = set(tc.reachable()), tc.instantiated()
    assert reach <= inst
    assert tc.table_tuples() == reach
    assert set(tc.PINNED) == inst - reach, sorted(set(tc.PINNED) ^ (inst - reach), key=str)
    assert all(len(r) > 20 for r in tc.PINNED.values())
    # what the issue names: the pair16 form, both splits, one and two polarisations, both input kinds, forced and by length
    assert ("p3", 12, True, False, True) in reach                    # k_inv_chan<12, 0, 2> on real input: pair16
    assert ("p3", 12, True, True, True) in reach and ("p3", 12, True, False, False) in reach
    cases = [c for c in tc.CASES if c["family"] in ("three", "four")]
    for key, values in (("real", (True, False)), ("npol", (1, 2)), ("sii", (True, False)), ("four", (0, 1)),
                        ("form", ("raw8", "float", "caspsr"))):
        assert {c[key] for c in cases} == set(values), key
    assert {c["M"] for c in cases if c["family"] == "four" and not c["four"]} >= {1 << k for k in range(14, 18)}
    # the two-pass path at both ends of every freq_res, k_fwd_col1q and every k_fwd_cols<lfa> the path takes
    two = {t for c in tc.CASES if c["family"] == "two" for t in c["picks"]["tuples"]}
    assert {("rinv", m) for m in range(9, 13)} <= two and ("col1q",) in two
    # every odd factor in either length, the compiled radices with both input kinds
    for fam, key in (("odd_C", "nsub"), ("odd_M", "msub")):
        got = {(c["picks"][key], c["real"]) for c in tc.CASES if c["family"] == fam}
        assert {r for r, _ in got} == set(tc.ODD_FACTORS)
        assert all((r, True) in got and (r, False) in got for r in tc.COMPILED_RADICES)
    assert {(tc._odd_part(c["C"]), tc._odd_part(c["M"])) for c in tc.CASES if c["family"] == "odd_CM"} == set(tc.ODD_PRODUCTS)
    assert {c["M"] for c in tc.CASES if c["family"] == "conv1"} == {1 << k for k in range(6, 14)}
    assert {c["family"] for c in tc.CASES if not c["kernel"] and not c["matrix"]} == set(tc.EXPECTED_PATH) - {"matrix", "odd_CM"}


@pytest.mark.parametrize("name", tc.NAMES)
def test_truth_and_baseline(oracle, name):
    b, T, f32 = tc.truth(name)
    c = b.case
    M, nkeep = c["M"], c["M"] - sum(c["nfilt"])
    assert f32["shape"] == (c["C"] * c["input_nchan"], c["npol"], c["npart"] * nkeep)
    assert f32["periodic"] <= 1e-12                                              # M-periodic over all parts
    A = tc.analytic_gains(b)
    amp = f32["amp"]
    assert math.sqrt(np.mean(np.abs(T - A) ** 2)) <= 1e-10 * amp
    # no weak bin: "relative to the rms amplitude" is within a factor 2 of "relative to the bin".  Not so behind a Jones matrix,
    # whose two terms cancel at some bins whatever the input (measured: down to 2e-3 of the rms): there the INPUT has no weak bin, and
    # the bounds of the GPU test are relative to the rms amplitude either way.
    weakest = np.abs(tc.analytic_gains(b, response=False)).min() / math.sqrt(np.mean(np.abs(tc.analytic_gains(b, response=False)) ** 2)) \
        if c["matrix"] else np.abs(T).min() / amp
    assert weakest >= 0.5, "a weak bin: %.3g of the rms" % weakest
    # the baseline the GPU test is judged against (transfer_cases.truth keeps it): positive, bin 0 part of it, and far enough below the
    # transform tolerance that four times it still is
    assert 0 < f32["rms"] <= f32["worst"] and f32["bin0"] <= f32["worst"]
    assert 4 * f32["worst"] <= tc.fb_tolerance(c), (f32, tc.fb_tolerance(c))
    print("%s f32: rms %.3g worst %.3g bin0 %.3g weakest bin %.3g" % (name, f32["rms"], f32["worst"], f32["bin0"], weakest))


# (C, M, real, form): the sizes the method was first tried at; the first is a case of the table
SENSITIVE = [(8, 64, True, "raw8"), (64, 1024, False, "float"), (256, 4096, True, "raw8")]


@pytest.mark.parametrize("C,M,real,form", SENSITIVE)
def test_one_response_bin_off_by_1e_5_is_found_where_it_is(oracle, C, M, real, form):
    c = tc.make_case("three", C, M, real, form=form)
    b = tc.block(oracle, c)
    ref = tc.reference(oracle, b, np.float64)
    T = tc.gains(ref, c)
    N = C * M
    tol = tc.fb_tolerance(c)
    base = tc.figures(tc.gains(tc.reference(oracle, b, np.float32), c), T)
    for k in (0, M * (C // 2), (N // 3) | 1, N - 1):                                 # bin 0, a channel's first, a mid bin, the last
        kern = b.kernel.copy()
        kern[k] *= np.complex64(1 + 1e-5)
        got = tc.reference(oracle, b, np.float32, kernel=kern)
        f = tc.figures(tc.gains(got, c), T)
        chan, m = divmod(k, M)
        assert f["where"][1] == chan and f["where"][3] == m, (k, f["where"])
        rel = f["worst"] * f["amp"] / np.abs(T[f["where"]])                          # relative to that bin's own gain
        assert 0.8e-5 <= rel <= 1.2e-5, (k, rel)
        assert f["worst"] > 4 * base["worst"]                                        # the GPU test's bound refuses it
        if m == 0:
            assert f["bin0"] == f["worst"]
        rms_err, max_err = tc.old_measures(got, ref)                                 # ... and _fb_case's two would not
        assert rms_err <= tol and max_err <= 8 * tol, (rms_err, max_err, tol)
        print("C=%d M=%d bin %d: %.3g at the bin; _fb_case rms %.3g (bound %.3g) max %.3g (bound %.3g)" %
              (C, M, k, rel, rms_err, tol, max_err, 8 * tol))
