"""Every filterbank output depends on its own input row and part only (tests/row_isolation_cases.py has the property, the table and the
perturbations; tests/test_row_isolation_cases_host.py shows that the oracles meet every equality asked here).  One ordinary call of
perform / perform_raw per run into plain rows, as tests/test_gpu_transfer.py makes; the baseline of a case runs once and is shared.
All comparisons are of int32 views.

Per case and perturbation (one test each; at most three targets, so at most three small calls beside the shared baseline):
  * locality: whatever the data flow says is unaffected is bit-identical to the baseline -- the other rows (`independent`), the other
    input channels (`paired`, matrix), the other parts (first, last, poison);
  * homogeneity, float rows: an independent target at 2^-12 gives the baseline x 2^-12, a dead one +-0, a silent part +-0 in every
    row, a poisoned part NaN;
  * global scale, 8-bit rows: perform_raw with scale x 2^-12 gives the baseline x 2^-12 -- no absolute constant inside a pass;
  * `paired` rows (real dual-polarisation input: W = X0 + i X1 in one transform): the error of each row of the pair against the
    float64 truth of the PERTURBED block, relative to the rms amplitude of the pair, within MARGIN of the float32 oracle's figures for
    that pair on the baseline block (the oracle pairs nothing, so the perturbation leaves its figures where they were), spread evenly
    over bin indices and channels.  Printed beside it: the same error relative to the row's OWN amplitude -- what the user of a
    weak or dead polarisation sees; profiles/HISTORY.md holds the table.  A pair whose partner comes back bit for bit is not a pair:
    the test fails with "listed as paired but independent"."""
import math

import numpy as np
import pytest

import row_isolation_cases as ric
import transfer_cases as tc
from test_gpu_transfer import MARGIN, SPREAD, fallback, run_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RUNS = [(c["name"], kind) for c in ric.CASES for kind in ric.KINDS if any(k == kind for k, _ in ric.runs(c))]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


_shared = {}


def shared(gpu, name):
    """the baseline block of a case, its device output and (lazily) the float32 oracle's figures per pair: once per case"""
    if _shared.get("name") != name:
        import oracle.dspsr_oracle as o
        b = ric.baseline(o, ric.by_name(name))
        base = run_case(gpu, b)
        assert np.isfinite(base.view(np.float32)).all() and ric.bits(base).any()
        _shared.clear()
        _shared.update(name=name, o=o, b=b, base=base, oracle_pairs=None)
    return _shared


def oracle_pairs(s):
    """the float32 oracle's pair_figures of every input channel on the baseline block"""
    if s["oracle_pairs"] is None:
        o, b = s["o"], s["b"]
        c = b.case
        T = tc.gains(tc.reference(o, b, np.float64), c)
        G = tc.gains(tc.reference(o, b, np.float32), c)
        s["oracle_pairs"] = [ric.pair_figures(G, T, c, i) for i in range(c["input_nchan"])]
    return s["oracle_pairs"]


def measure_pair(s, p, got, kind, target):
    """the paired rows of the target's input channel against the float64 truth of the perturbed block"""
    o, b = s["o"], s["b"]
    c = b.case
    i = ric.target_rows(c, target)[0][0]
    f32 = oracle_pairs(s)[i]
    T = tc.gains(tc.reference(o, p, np.float64), c)
    pf = ric.pair_figures(tc.gains(got, c), T, c, i)
    fb = fallback(c)
    tol = tc.fb_tolerance(c)
    for pol, r in enumerate(pf["rows"]):
        by_m, at_m, by_s, at_s, n_m, n_s = tc.structure(r["err"])
        own = r["rms"] * pf["amp"] / r["own"] if r["own"] > 0 else math.inf
        print("PAIR %s %s %s row (%d, %d): e_r %.3g worst %.3g of the pair (amplitude %.3g); e_r %.3g of its own amplitude %.3g; f32 pair "
              "rms %.3g worst %.3g; ratios rms %.2f worst %.2f; spread m %.2f s %.2f" %
              (c["name"], kind, "%s%d" % target, i, pol, r["rms"], r["worst"], pf["amp"], own, r["own"], f32["rms"], f32["worst"],
               r["rms"] / f32["rms"], r["worst"] / f32["worst"], by_m, by_s))
        where = "%s %s %s, row (%d, %d)" % (c["name"], kind, target, i, pol)
        if fb is None or not fb[1]:
            assert r["rms"] <= MARGIN * f32["rms"], "%s: error rms %.3g of the pair > %d x %.3g" % (where, r["rms"], MARGIN, f32["rms"])
        if fb is None:
            assert r["worst"] <= MARGIN * f32["worst"], "%s: worst bin %.3g of the pair > %d x %.3g" % (where, r["worst"], MARGIN,
                                                                                                       f32["worst"])
        else:
            assert r["worst"] <= tol, "%s: worst bin %.3g of the pair > %.3g (%s)" % (where, r["worst"], tol, fb[0])
        # (a group of fewer than 8 samples says nothing about its rms)
        assert n_m < 8 or by_m <= SPREAD, "%s: bin index %d carries %.2f times the error rms of the row" % (where, at_m, by_m)
        assert n_s < 8 or by_s <= SPREAD, "%s: channel %d carries %.2f times the error rms of the row" % (where, at_s, by_s)


@pytest.mark.parametrize("name,kind", RUNS)
def test_outputs_depend_on_their_own_row_and_part(gpu, name, kind):
    s = shared(gpu, name)
    o, b, base = s["o"], s["b"], s["base"]
    c = b.case
    paired = c["rows"] == "paired"
    for k, target in ric.runs(c):
        if k != kind:
            continue
        p = ric.perturbed(o, b, kind, target)
        got = run_case(gpu, p)
        n = ric.check_equalities(b, base, got, kind, target, paired)
        print("%s %s %s: %d floats held bit for bit" % (name, kind, target, n))
        if kind not in ("other", "weak", "dead") or target[0] != "pol" or c["npol"] != 2:
            continue
        assert not np.array_equal(ric.bits(got), ric.bits(base)), "the perturbation changed nothing"
        if paired:
            assert np.isfinite(got.view(np.float32)).all()
            if not c["matrix"]:
                assert not ric.partner_unchanged(b, base, got, target), \
                    "%s %s %s: listed as paired but independent (the partner came back bit for bit)" % (name, kind, target)
                if ric.is_float(c) and kind == "weak":
                    m = ric.expand(b, ric.target_mask(b, target), range(c["npart"]))
                    want = np.ldexp(base.view(np.float32), ric.WEAK_LOG2).view(np.complex64)
                    assert not np.array_equal(ric.bits(want)[np.repeat(m, 2, axis=2)], ric.bits(got)[np.repeat(m, 2, axis=2)]), \
                        "%s weak %s: listed as paired but independent (the target is the baseline x 2^%d exactly)" % (
                            name, target, ric.WEAK_LOG2)
            measure_pair(s, p, got, kind, target)
