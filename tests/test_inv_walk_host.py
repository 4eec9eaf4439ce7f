"""The work items of the inverse passes k_inv_chan and k_rows_inv (dspsr_amd/csrc/fb_inv_walk.h: plain integer arithmetic, the
workgroup index and the grid size as arguments), checked without a GPU.

tests/inv_walk_driver.cpp includes only that header; it is built with g++ and the address and undefined-behaviour sanitizers and
run as a stand-alone program (nothing is loaded into Python).  For one launch per line it walks every workgroup's items and checks
that every (tile, part) of the launch is dealt exactly once and nothing else, that a workgroup's sequence ends at its first `false`,
and for the ordered walks (fused fold, search mode) that one workgroup takes the parts of a (tile, run of parts) in ascending order
and that run s holds the parts [s * pps, min(nparts, (s + 1) * pps)).

The launches are the ones the host forms (filterbank.hip): grids of grid_for on 8, 64, 256 and 512 workgroups, run == nparts
(fb_run_tiles, fb_run_two_pass), and for the segmented fused fold the nseg of fb_launch_fused with grid = tiles * nseg."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WGS = (8, 64, 256, 512)
NTILE = (1, 2, 3, 5, 7, 8, 9, 12, 16, 24, 31, 32, 33, 63, 64, 65, 100, 128, 200, 255, 256, 257, 300)
NPARTS = (1, 2, 3, 5, 8, 13, 16, 31, 32, 100, 128, 255, 256)


def grid_for(items, ncu):
    g = min(items, ncu)
    return g & ~7 if g >= 8 else g


def fused_nseg(tiles, wgs, ns):
    """fb_launch_fused: runs of a segmented fold"""
    return max(1, min(wgs // tiles, ns, 16)) if tiles < wgs else 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("inv_walk") / "inv_walk_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "dspsr_amd", "csrc"), os.path.join(ROOT, "tests", "inv_walk_driver.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr.strip() == "", p.stderr[-4000:]              # -Wall -Wextra clean

    def run(lines):
        text = "".join(" ".join(str(int(v)) for v in l) + "\n" for l in lines)
        p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-4000:])
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
        bad = [(l, v) for l, v in zip(lines, out) if v != "ok"]
        assert not bad, bad[:10]
    return run


# a line: (ordered, matrix, nseg, nparts, ntile, run, grid, xcd_lr)

def test_free_order_of_the_plain_output(driver):
    # EPI == 0: one item per (tile, part); the scalar and the matrix response (another tile-major rule)
    driver([(0, matrix, 1, nparts, ntile, nparts, grid_for(ntile * nparts, wgs), 0)
            for wgs in WGS for ntile in NTILE for nparts in NPARTS for matrix in (0, 1)])


def test_search_mode_one_workgroup_per_tile(driver):
    driver([(1, 0, 1, nparts, ntile, nparts, grid_for(ntile, wgs), 0) for wgs in WGS for ntile in NTILE for nparts in NPARTS])


def test_fused_fold_exact_order(driver):
    # nseg == 1; xcd_lr = logX3 - logT3 of k_inv_chan (tiles of one X layout block on one XCD), 0 for k_rows_inv
    driver([(1, 0, 1, nparts, ntile, nparts, grid_for(ntile, wgs), lr)
            for wgs in WGS for ntile in NTILE for nparts in NPARTS for lr in (0, 1, 2, 3)])


def test_fused_fold_segmented(driver):
    lines = []
    for wgs in WGS:
        for ntile in NTILE:
            for nparts in NPARTS:
                nseg = fused_nseg(ntile, wgs, nparts)
                if nseg > 1:
                    lines += [(1, 0, nseg, nparts, ntile, nparts, ntile * nseg, lr) for lr in (0, 1)]
    assert {l[2] for l in lines} >= {2, 3, 5, 8, 13, 16}          # (runs that do and do not divide the parts)
    driver(lines)


def test_every_nseg_up_to_16(driver):
    # every nseg the host can form, also where the last runs are empty (nparts = 5, nseg = 4: pps = 2, run 3 has no part)
    driver([(1, 0, nseg, nparts, ntile, nparts, ntile * nseg, 0)
            for nseg in range(1, 17) for nparts in range(nseg, 40) for ntile in (1, 3, 8, 31)])


def test_runs_the_host_does_not_pass(driver):
    # the XCD dealing's general branch (run != nparts): no launch of the library takes it
    driver([(0, 0, 1, nparts, ntile, run, grid_for(ntile * nparts, wgs), 0)
            for wgs in (8, 64, 250) for ntile in (1, 7, 64, 100) for nparts in (1, 3, 32, 100) for run in (1, 4, 32)])
