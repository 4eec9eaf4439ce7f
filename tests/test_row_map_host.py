"""The mirror-paired row order of the pre-split spectrum (dspsr_amd/csrc/fb_row_map.h: plain integer arithmetic shared by pass 1's
copy-out, pass 2 and the host dispatch), checked without a GPU.

tests/row_map_driver.cpp includes only that header; it is built with g++ and the address and undefined-behaviour sanitizers and
run as a stand-alone program (nothing is loaded into Python).  For every (logM, logT2) with 1 <= logT2 <= logM <= 13 -- every
pass-2 tile the three-pass path can have -- it checks that (block, slot) -> row is a bijection with rm_slot as its inverse, that
each block holds every row together with its mirror M - row in the slot rm_mirror names, that rows 0 and M / 2 sit in block 0,
and that the halves of a block are runs of adjacent rows; and that the X' index is a bijection that keeps the channels of a layout
block adjacent."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("row_map") / "row_map_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "dspsr_amd", "csrc"), os.path.join(ROOT, "tests", "row_map_driver.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr.strip() == "", p.stderr[-4000:]              # -Wall -Wextra clean

    def run(lines):
        text = "".join(" ".join(str(v) for v in l) + "\n" for l in lines)
        p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-4000:])
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def test_every_tile_height_of_every_transform_length(driver):
    # (the X' layout: two channels per block as at the headline, and one block for all channels; 8 channels keep the walk short)
    lines = [(logM, logT2, logX3, 3) for logM in range(1, 14) for logT2 in range(1, logM + 1) for logX3 in (1, 3)]
    for l, verdict in zip(lines, driver(lines)):
        assert verdict == "ok", (l, verdict)


def test_the_headline_blocks(driver):
    # -F 1024:D -x 4096: M = 4096, T2 = 8, T3 = X3 = 2, C = 1024
    assert driver([(12, 3, 1, 10)]) == ["ok"]
