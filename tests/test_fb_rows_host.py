"""The filterbank's row-overlap rule (dspsr_amd/csrc/fb_rows.h: pure host C++, standard headers only), which perform / perform_raw,
perform_detect and perform_search ask before they write a row.

tests/fb_rows_driver.cpp includes only that header; it is built with g++ and the address and undefined-behaviour sanitizers and run as
a stand-alone program (nothing is loaded into Python).  Every case with 1..3 outer indices (channels), 1..3 inner ones (polarisations
or planes), rows of 0..4 floats and both strides in 0..12 is asked:

  sound       whenever a predicate accepts, the nouter * ninner intervals [o * outer + i * inner, + row) are pairwise disjoint
  unchanged   the answers for the three callers are those of the expressions the callers held before the rule had a header of its own
              (filterbank.hip at commit 4ab53fe: fb_complex_rows_ok, perform_detect, perform_search), transcribed below
"""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(no, ni, so, si, row) for no, ni, row, so, si in
         itertools.product(range(1, 4), range(1, 4), range(0, 5), range(0, 13), range(0, 13))]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """one (outer_major, inner_major, ok either order, ok outer-major only, the same two for a call that writes nothing) per case"""
    exe = tmp_path_factory.mktemp("fb_rows") / "fb_rows_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "dspsr_amd", "csrc"), os.path.join(ROOT, "tests", "fb_rows_driver.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr.strip() == "", p.stderr[-4000:]              # -Wall -Wextra clean
    text = "".join("%d %d %d %d %d\n" % c for c in CASES)
    p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-4000:])
    out = [tuple(int(v) for v in line.split()) for line in p.stdout.splitlines()]
    assert len(out) == len(CASES) and all(len(a) == 6 for a in out)
    return out


def _disjoint(no, ni, so, si, row):
    """brute force: no float belongs to two rows"""
    seen = set()
    for o in range(no):
        for i in range(ni):
            cells = set(range(o * so + i * si, o * so + i * si + row))
            if seen & cells:
                return False
            seen |= cells
    return True


def test_an_accepted_layout_has_disjoint_rows(answers):
    assert len(CASES) == 3 * 3 * 5 * 13 * 13
    accepted = [0, 0]
    for case, a in zip(CASES, answers):
        for k in (0, 1):
            if a[k]:
                accepted[k] += 1
                assert _disjoint(*case), (case, "outer-major" if k == 0 else "inner-major")
    assert min(accepted) > 500                                   # both predicates accept a good part of the cases
    # and neither is the other: a layout only the inner-major order has, and one only the outer-major order has
    assert answers[CASES.index((2, 2, 4, 8, 4))][:2] == (0, 1) and answers[CASES.index((2, 2, 8, 4, 4))][:2] == (1, 0)


# ---- the callers' expressions at commit 4ab53fe (dspsr_amd/csrc/filterbank.hip), each returning "the call is refused" --------------
def _parent_complex(npart, nchan_out, npol, out_chan_stride, out_pol_stride, row):
    """fb_complex_rows_ok (perform, perform_raw); row = (npart - 1) * out_step + 2 * nkeep there, 0 for npart 0"""
    chan_major = (npol == 1 or out_pol_stride >= row) and (nchan_out == 1 or out_chan_stride >= (npol - 1) * out_pol_stride + row)
    pol_major = npol > 1 and (nchan_out == 1 or out_chan_stride >= row) and out_pol_stride >= (nchan_out - 1) * out_chan_stride + row
    return bool(npart and not chan_major and not pol_major)


def _parent_detect(npart, nchan_out, planes, det_chan_stride, det_pol_stride, row):
    """perform_detect; planes = 4 / ndim and row = npart * nkeep * ndim there"""
    chan_major = (planes == 1 or det_pol_stride >= row) and (nchan_out == 1 or det_chan_stride >= (planes - 1) * det_pol_stride + row)
    plane_major = planes > 1 and (nchan_out == 1 or det_chan_stride >= row) and det_pol_stride >= (nchan_out - 1) * det_chan_stride + row
    return bool(npart and not chan_major and not plane_major)


def _parent_search(nout, nchan_out, npo, out_chan_stride, out_pol_stride):
    """perform_search: rows of the nout samples the call completes"""
    return bool(nout and ((npo > 1 and out_pol_stride < nout) or (nchan_out > 1 and out_chan_stride < (npo - 1) * out_pol_stride + nout)))


def test_the_three_callers_accept_what_they_accepted(answers):
    refused = [0, 0, 0]
    for (no, ni, so, si, row), (_om, _im, either, outer_only, either_none, outer_none) in zip(CASES, answers):
        case = (no, ni, so, si, row)
        # a call of one or more parts whose rows span `row` floats (npart enters the expressions as a flag only)
        assert either == (not _parent_complex(1, no, ni, so, si, row)), case
        assert either == (not _parent_detect(1, no, ni, so, si, row)), case
        # a call of no parts is never refused, whatever it says of its rows
        assert either_none == 1 and not _parent_complex(0, no, ni, so, si, row) and not _parent_detect(0, no, ni, so, si, row), case
        # search mode: row IS the number of completed samples, so "writes nothing" is row 0
        assert (outer_only if row else outer_none) == (not _parent_search(row, no, ni, so, si)), case
        assert outer_none == 1, case
        refused[0] += not either
        refused[1] += not outer_only
        refused[2] += bool(either and not outer_only)
    assert min(refused) > 100                                    # refusals on both forms, and layouts the search form alone refuses
