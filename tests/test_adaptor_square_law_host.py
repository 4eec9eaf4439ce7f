"""HIP::DetectionEngine::square_law in the deferred HIP::Chain (dspsr -d 1, -d 2, one input polarisation), without a GPU:
tests/adaptor_square_law_driver.cpp drives Filterbank -> Detection::square_law -> Fold over the recording C-ABI of
tests/capi_recorder.cpp against the miniatures of tests/host_mock; its log -- the ordered C-ABI calls with their arguments, the
Errors, the chain's counters -- must equal tests/golden/adaptor_square_law/chain_square_law.txt.  Recorded and fused: Intensity,
PPQQ and one polarisation behind a recorded filterbank block (ONE dspsr_amd_filterbank_perform_fold with state 2 / 3 / 2).
Eager, as before: a chain that is not deferred, a finish() in between, a fold of a piece, an output state or a profile shape
the fused fold does not write; and a later reader of a fused block's rows is refused."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adaptor_square_law", "chain_square_law.txt")


def _log(tmp_path):
    exe = os.path.join(str(tmp_path), "adaptor_square_law_driver")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wno-unused-function", "-Wno-reorder", "-I", os.path.join(ROOT, "tests", "host_mock"),
           "-I", os.path.join(ROOT, "dspsr_amd", "host"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests"),
           os.path.join(ROOT, "tests", "adaptor_square_law_driver.cpp"), os.path.join(ROOT, "tests", "capi_recorder.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    out = os.path.join(str(tmp_path), "chain_square_law.txt")
    p = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return open(out).read().splitlines()


def test_square_law_chain_trace(tmp_path):
    got, want = _log(tmp_path), open(GOLDEN).read().splitlines()
    for n, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, "line %d:\n  now      %s\n  recorded %s" % (n, g, w)
    assert len(got) == len(want)


def test_the_trace_says_what_is_fused(tmp_path):
    """the fixture itself: three recorded chains end in one perform_fold each with the state of the square law and launch no
    filterbank or detection of their own; the five eager ones launch dspsr_amd_detect_square_law and no perform_fold"""
    text = open(GOLDEN).read()
    parts = text.split("\n## ")
    assert len(parts) == 9
    for part, state, n in zip(parts[:3], (2, 3, 2), (2, 1, 1)):
        assert part.count("dspsr_amd_filterbank_perform_fold (") == n and part.count(", %d, fold" % state) == n
        assert "dspsr_amd_detect_square_law" not in part and "dspsr_amd_filterbank_perform (" not in part and "dspsr_amd_fold_fold (" not in part
    for part in parts[3:8]:
        assert "dspsr_amd_filterbank_perform_fold" not in part and part.count("dspsr_amd_detect_square_law (") == 1
        assert part.count("dspsr_amd_filterbank_perform (") == 1 and part.count("dspsr_amd_fold_fold (") == 1
    assert "Error InvalidState: HIP::DetectionEngine::square_law: this TimeSeries is an intermediate" in parts[8]
