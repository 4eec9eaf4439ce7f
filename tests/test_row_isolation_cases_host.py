"""tests/row_isolation_cases.py without a GPU: the float32 and the float64 oracle meet every equality tests/test_gpu_row_isolation.py
asks of the device -- on these inputs the reference's data flow alone satisfies them, with NO pairing of rows: the oracle transforms
every polarisation on its own, so the other polarisation of a target comes back bit for bit and a dead float row gives exact zeros
(what a `paired` device path gives up).  And the table's invariants: every coupling site is present, every case says which kind of rows
it has, every `paired` case cites where two rows enter one transform, and the names are unique."""
import numpy as np
import pytest

import row_isolation_cases as ric
import transfer_cases as tc

SITES = {
    "real2 pre-split", "real2 split in inverse", "real2 four passes forced", "real2 caspsr", "real2 float rows", "real2 full tile",
    "real2 four passes by length", "real2 odd_C", "real2 odd_M", "real2 subbands", "real2 matrix pre-split",
    "real2 matrix split in inverse", "real1", "complex2", "complex1", "complex2 four passes forced", "complex1 four passes forced",
    "complex2 two passes", "complex2 subbands float",
    "complex2 batched", "complex2 matrix", "conv1 short", "conv1 long", "conv3", "plain raw8", "plain float",
}


def test_table():
    assert len(set(ric.NAMES)) == len(ric.NAMES) and len(set(ric.SITES)) == len(ric.SITES)
    assert SITES <= set(ric.SITES)
    assert 24 <= len(ric.CASES) <= 34
    twins = {c["family"] for c in ric.CASES if not c["kernel"] and not c["matrix"]}
    assert twins >= {"three", "two", "odd_C", "subbands", "plain", "conv1", "batched"}
    for c in ric.CASES:
        assert c["rows"] in ("independent", "paired"), c["name"]
        assert c["picks"]["path"] in tc.EXPECTED_PATH[c["family"]], c["name"]
        # what reading the code says is paired is what the table lists as paired; anything further would need its own citation
        assert (c["rows"] == "paired") == ric.pairs_by_construction(c), c["name"]
        assert (c["rows"] == "paired") == bool(c["where"]), c["name"]
        if c["where"]:
            assert ".h:" in c["where"] or ".hip:" in c["where"], c["name"]
        # a full launch group and a ragged one; no length above 2^15 but the four-pass-by-length case
        assert c["max_parts"] == 2 and c["npart"] % 2 == 1 or c["M"] == 1, c["name"]
        assert c["picks"]["L"] <= 1 << 15 or c["site"] == "real2 four passes by length", c["name"]
        kinds = {k for k, _ in ric.runs(c)}
        assert kinds >= {"first", "last"} and (kinds >= {"other", "weak", "dead"} or ric.alone(c))
        assert ("poison" in kinds) == ric.is_float(c) and ("scale" in kinds) == (not ric.is_float(c))
    by_site = dict(zip(ric.SITES, ric.CASES))
    assert by_site["real2 pre-split"]["picks"]["presplit"] and not by_site["real2 split in inverse"]["picks"]["presplit"]
    assert by_site["real2 four passes by length"]["picks"]["passes"] == 4 and not by_site["real2 four passes by length"]["four"]
    assert by_site["real2 full tile"]["picks"]["tuples"][-1][2]
    assert by_site["real2 subbands"]["input_nchan"] == 2 and by_site["complex2 batched"]["input_nchan"] == 4


def test_the_perturbations_change_what_they_say_and_nothing_else(oracle):
    for name in ("three-16x256-r2-raw8", "three-16x256-r2-caspsr", "subbands-32x128-c2-float-in4"):
        c = ric.by_name(name)
        b = ric.baseline(oracle, c)
        step, fft, ndim = b.plan.nsamp_step, b.plan.nsamp_fft, b.obs.ndim
        for kind, target in ric.runs(c):
            p = ric.perturbed(oracle, b, kind, target)
            diff = ric.bits(p.rows.astype(np.float64)) != ric.bits(b.rows.astype(np.float64))
            diff |= np.isnan(p.rows)
            if kind == "scale":
                assert np.array_equal(p.raw, b.raw) and np.array_equal(p.rows, np.ldexp(b.rows, ric.WEAK_LOG2))
                continue
            rows = ric.target_mask(b, target)
            assert not diff[~rows].any(), (name, kind, target)
            lo, hi = {"first": (0, step), "last": (b.ndat - step, b.ndat), "silent": (step, step + fft),
                      "poison": (ric.poison_sample(b), ric.poison_sample(b) + 1)}.get(kind, (0, b.ndat))
            assert not diff[:, :, :lo * ndim].any() and not diff[:, :, hi * ndim:].any(), (name, kind)
            changed = diff[rows][:, lo * ndim:hi * ndim].mean()
            assert changed > (0.5 if kind in ("other", "weak", "dead", "first", "last") else 0), (name, kind, changed)
            if kind == "weak":
                ratio = p.rows[rows].astype(np.float64).std() / b.rows[rows].astype(np.float64).std()
                assert (ratio == 2.0 ** ric.WEAK_LOG2) if ric.is_float(c) else (0.1 <= ratio <= 0.15), ratio
            if kind == "dead" and not ric.is_float(c):
                assert (p.rows[rows] == np.float32(0.5) * np.float32(b.scale)).all()
            if b.raw is not None:
                assert np.array_equal(oracle.unpack_8bit(p.raw, b.obs, b.scale), p.rows)


@pytest.mark.parametrize("name", ric.NAMES)
def test_the_oracles_keep_every_row_to_itself(oracle, name):
    c = ric.by_name(name)
    b = ric.baseline(oracle, c)
    for dtype in (np.float32, np.float64):
        base = tc.reference(oracle, b, dtype)
        assert np.isfinite(base.view(base.real.dtype)).all() and ric.bits(base).any()
        nfloat = 0
        for kind, target in ric.runs(c):
            p = ric.perturbed(oracle, b, kind, target)
            with np.errstate(invalid="ignore"):
                got = tc.reference(oracle, p, dtype)
            n = ric.check_equalities(b, base, got, kind, target, paired=False)
            # (a matrix response leaves nothing of its one input channel untouched: those runs are measured on the device only)
            assert n > 0 or (c["matrix"] and c["rows"] == "paired" and kind in ("other", "weak", "dead")), (kind, target)
            nfloat += n
            if kind in ("other", "weak", "dead") and target[0] == "pol":
                assert not np.array_equal(ric.bits(got), ric.bits(base))                 # the run changed something
                if c["npol"] == 2 and not c["matrix"]:
                    assert ric.partner_unchanged(b, base, got, target)
        print("%s %s: %d runs, %d floats held" % (name, np.dtype(dtype).name, len(ric.runs(c)), nfloat))


def test_pair_figures_are_those_of_transfer_cases_on_equal_rows(oracle):
    """on a baseline block (equal amplitudes) the pair's figures are transfer_cases.figures' of the whole output"""
    c = ric.by_name("three-16x256-r2-raw8")
    b = ric.baseline(oracle, c)
    T = tc.gains(tc.reference(oracle, b, np.float64), c)
    G = tc.gains(tc.reference(oracle, b, np.float32), c)
    f32 = tc.figures(G, T)
    pf = ric.pair_figures(G, T, c, 0)
    assert abs(pf["rms"] / f32["rms"] - 1) < 1e-9 and abs(pf["worst"] / f32["worst"] - 1) < 1e-9
    assert abs(pf["amp"] / f32["amp"] - 1) < 1e-9
    for r in pf["rows"]:
        assert 0.8 < r["rms"] / pf["rms"] < 1.25 and abs(r["own"] / pf["amp"] - 1) < 0.05
