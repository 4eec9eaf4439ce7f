"""Every path through the pipeline drivers (tools/pipeline_paths.py) against tests/golden/pipeline_paths.json: the host arithmetic
each path leaves behind -- derived attributes, counters after each block, the books of every sub-integration, the operations timed and
their call counts -- for exact equality (floats as float.hex()).  The fixture was recorded with the same tool from the commit in front
of the one that gave LoadToFold a single constructor path (the last four search cases: from the commit in front of the one that
built the search drivers from front ends and output stages); it holds no profile samples (the path tests pin those against the oracle)."""
import importlib.util
import json
import os

import pytest

from dspsr_amd import pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("pipeline_paths", os.path.join(ROOT, "tools", "pipeline_paths.py"))
paths = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(paths)

with open(os.path.join(ROOT, "tests", "golden", "pipeline_paths.json")) as _f:
    GOLDEN = json.load(_f)

CASES = ["during_fused", "during_L", "during_K", "during_subband_K", "after", "never", "before", "cyclic", "plfb", "two_targets_s",
         "fourth_moment", "coherent_fused", "coherent_K_f", "direct_K", "fil", "coherent_d4", "fits_F_D", "fits_direct_K"]


def test_the_fixture_holds_every_case():
    assert sorted(GOLDEN) == sorted(CASES) == sorted(paths.case_names(pipeline))
    # what the cases are there for: a boundary inside the second block, a fused and an unfused block, a rank that gives samples up
    assert len(GOLDEN["during_L"]["subints"][""]) == 2 and GOLDEN["during_L"]["optime"]["Filterbank+Detection"] == 1
    assert GOLDEN["during_fused"]["optime"] == {"Filterbank+Detection+Fold": 3} and GOLDEN["during_fused"]["attrs"]["fused_mode"] == 1
    assert GOLDEN["during_K"]["attrs"]["sd_head"] > 0 and GOLDEN["during_subband_K"]["attrs"]["in_nchan"] == 1
    assert sorted(GOLDEN["two_targets_s"]["subints"]) == ["a", "b"] and all(len(v) > 1 for v in GOLDEN["two_targets_s"]["subints"].values())
    assert GOLDEN["fourth_moment"]["optime"]["Fold"] == 4 and len(GOLDEN["fourth_moment"]["subints"][""]) == 2


@pytest.mark.parametrize("name", CASES)
def test_path_keeps_its_host_arithmetic(name):
    rec, arrays = paths.run_case(pipeline, name)
    rec = json.loads(json.dumps(rec))                     # (tuples to lists, as the fixture went through JSON)
    want = GOLDEN[name]
    for key in sorted(set(want) | set(rec)):
        assert rec.get(key) == want.get(key), (name, key)
    assert arrays and all(a.size for a in arrays.values())
