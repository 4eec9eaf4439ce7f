"""The layout of the regrouped 8-bit input (dspsr_amd/csrc/fb_rt_layout.h: plain integer arithmetic shared by k_raw_transpose,
pass 1 and the host dispatch), checked without a GPU.

tests/rt_layout_driver.cpp includes only that header; it is built with g++ and the address and undefined-behaviour sanitizers and
run as a stand-alone program (nothing is loaded into Python).  For every geometry it walks all (part, sequence, tile, row, column)
and reports the first property that fails (see the driver's header): offsets inside the allocation, distinct places for distinct
rows, one place for a row that several parts share, 2*T1-byte pieces and 16-byte two-row stores.

Geometries: those of tests/test_gpu_shared_regroup.py (5 parts with max_parts 4: a shared group of four, then a group of one)
and the headline's launch group (-F 1024:D -x 4096 at DM 1000, 32 parts); real dual-pol input, so a row is Rr = 2 C samples and
the tiles have T1 = min(Rr, 2^14 / M) columns (filterbank.hip fb_tile)."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_BLOCK = 64

# (C, M, nfilt, parts of the group, parts allocated)
GEOMETRIES = [
    (4, 4096, (422, 422), 4, 4),        # four-column tiles, nkeep even
    (4, 4096, (421, 422), 4, 4),        # nkeep odd: odd row shifts, odd row count
    (16, 256, (20, 21), 4, 4),          # wide tiles
    (4, 8192, (100, 101), 4, 4),        # two-column tiles
    (2, 2048, (100, 50), 4, 4),         # Rr < 8
    (4, 16, (1, 2), 4, 4),              # windows shorter than a row block
    (1024, 4096, (422, 422), 32, 32),   # the headline's launch group
    (4, 4096, (422, 422), 1, 4),        # a group of one part: per part
    (4, 4096, (422, 422), 2, 4),
    (4, 16, (1, 2), 2, 4),              # two short windows: the padded grid would be larger than two windows, per part
]


def _line(C, M, nfilt, nb, alloc, part_step=None):
    logM, logR = int(math.log2(M)), int(math.log2(2 * C))
    logT1 = min(logR, 14 - logM)
    nkeep = M - sum(nfilt)
    step = nkeep * 2 * C if part_step is None else part_step
    return (logM, logR, logT1, 1, nb, step, alloc), nkeep


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rt_layout") / "rt_layout_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "dspsr_amd", "csrc"), os.path.join(ROOT, "tests", "rt_layout_driver.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr.strip() == "", p.stderr[-4000:]              # -Wall -Wextra clean

    def run(lines):
        text = "".join(" ".join(str(v) for v in l) + "\n" for l in lines)
        p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-4000:])
        out = p.stdout.splitlines()
        assert len(out) == 2 * len(lines)
        return [(tuple(int(v) for v in out[2 * i].split()), out[2 * i + 1]) for i in range(len(lines))]
    return run


def test_layout_properties_hold_for_every_geometry(driver):
    lines, nkeeps = zip(*(_line(*g) for g in GEOMETRIES))
    for g, l, nkeep, ((shared, rows, padded, elems, alloc), verdict) in zip(GEOMETRIES, lines, nkeeps, driver(lines)):
        C, M, _nfilt, nb, _ = g
        assert verdict == "ok", (g, verdict)
        want_rows = nkeep * (nb - 1) + M
        want_shared = nb > 1 and -(-want_rows // ROW_BLOCK) * ROW_BLOCK <= nb * M
        assert shared == want_shared, g
        if shared:
            assert (rows, padded) == (want_rows, -(-want_rows // ROW_BLOCK) * ROW_BLOCK) and elems == 2 * C * padded <= alloc, g
        else:
            assert (rows, padded, elems) == (M, M, nb * 2 * C * M), g
    # the headline: 104908 rows regrouped per 32 parts instead of 131072
    assert driver([lines[6]])[0][0][:3] == (1, 104908, 104960)
    assert [driver([l])[0][0][0] for l in (lines[7], lines[8], lines[9])] == [0, 1, 0]


def test_two_sequences_have_a_grid_each(driver):
    # complex dual-pol input, C = 32, M = 128: Rr = 32, one sequence per polarisation; 4 parts 109 rows apart
    (got, verdict), = driver([(7, 5, 5, 2, 4, 109 * 32, 4)])
    rows = 109 * 3 + 128
    assert verdict == "ok" and got[:3] == (1, rows, -(-rows // ROW_BLOCK) * ROW_BLOCK) and got[3] == 2 * 32 * got[2]


@pytest.mark.parametrize("part_step,shared", [
    (3252 * 8, 1),          # whole rows
    (3252 * 8 + 4, 0),      # not a multiple of Rr = 8: per part
    (4096 * 8, 1),          # windows that touch: nothing shared, nothing lost
    (4097 * 8, 0),          # windows apart: the grid would hold rows nobody reads, and be larger than the allocation
    (0, 0),
])
def test_part_steps_off_the_row_grid_take_the_per_part_form(driver, part_step, shared):
    line, _ = _line(4, 4096, (422, 422), 4, 4, part_step=part_step)
    (got, verdict), = driver([line])
    assert verdict == "ok" and got[0] == shared
