"""What the adaptor headers of dspsr_amd/host make of DSPSR's engine calls, without a GPU: tests/adaptor_trace_driver.cpp drives
every adaptor class over the recording C-ABI of tests/capi_recorder.cpp (plain C++, no -ldspsr_amd) against the miniatures of
tests/host_mock, and writes per scenario the ordered C-ABI calls with their arguments, the Errors thrown (code, method, message)
and the counters of the HIP::Chain.  Each log must equal tests/golden/adaptor_trace/<scenario>.txt.

The fixtures are the behaviour contract of the adaptors: the order and the arguments of every library call, every transition of
the deferred chain, every stride.  They were recorded from the headers as they stood before the deferred-chain state machine moved
into HIP::Chain; `python tests/test_adaptor_trace_host.py --regenerate` rewrites them from the headers of the tree.
DSPSR_AMD_HOST_HEADERS names another directory of host headers to build against (an export of an earlier commit, say): the same
fixtures must hold there.  One case stands outside the fixtures and is always built against the headers of the tree: a library
message that holds a printf conversion must reach the Error as it is (the headers the fixtures were recorded from handed the
message to Error as its format in two of three places, and print a stray number for "%d")."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adaptor_trace")
TREE_HEADERS = os.path.join(ROOT, "dspsr_amd", "host")
HEADERS = os.environ.get("DSPSR_AMD_HOST_HEADERS") or TREE_HEADERS
SCENARIOS = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt")) if os.path.isdir(GOLDEN) else []


def _build_driver(directory, headers=HEADERS):
    exe = os.path.join(str(directory), "adaptor_trace_driver")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wno-unused-function", "-Wno-reorder", "-I", os.path.join(ROOT, "tests", "host_mock"),
           "-I", headers, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests"),
           os.path.join(ROOT, "tests", "adaptor_trace_driver.cpp"), os.path.join(ROOT, "tests", "capi_recorder.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def _record(directory, into):
    exe = _build_driver(directory)
    os.makedirs(into, exist_ok=True)
    p = subprocess.run([exe, into], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return exe


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    directory = tmp_path_factory.mktemp("adaptor_trace")
    out = os.path.join(str(directory), "logs")
    exe = _record(directory, out)
    return exe, out


def test_every_scenario_has_its_fixture(recorded):
    _, out = recorded
    assert SCENARIOS, "no fixtures under tests/golden/adaptor_trace"
    assert sorted(f[:-4] for f in os.listdir(out)) == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_adaptor_trace(recorded, scenario):
    _, out = recorded
    with open(os.path.join(out, scenario + ".txt")) as f:
        got = f.read().splitlines()
    with open(os.path.join(GOLDEN, scenario + ".txt")) as f:
        want = f.read().splitlines()
    for n, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, "%s line %d:\n  now      %s\n  recorded %s" % (scenario, n, g, w)
    assert len(got) == len(want), "%s: %d lines now, %d recorded" % (scenario, len(got), len(want))


def test_library_message_is_not_a_format(recorded, tmp_path):
    exe = recorded[0] if HEADERS == TREE_HEADERS else _build_driver(tmp_path, TREE_HEADERS)
    p = subprocess.run([exe, "--messages"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "messages ok" in p.stdout, p.stdout + p.stderr


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_adaptor_trace_host.py --regenerate")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for name in os.listdir(GOLDEN) if os.path.isdir(GOLDEN) else []:
            if name.endswith(".txt"):
                os.remove(os.path.join(GOLDEN, name))
        _record(tmp, GOLDEN)
    print("wrote %d fixtures to %s from %s" % (len(os.listdir(GOLDEN)), GOLDEN, HEADERS))
