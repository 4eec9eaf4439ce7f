"""HIP::MatrixFilterbankEngine (dspsr_amd/host/dspsr_amd_matrix_engine.h): the filterbank adaptor for responses that may be
matrix responses.  tests/matrix_adaptor_driver.cpp is built against the miniatures of tests/host_mock (its dsp::Response has
get_ndim (), as the real one has through Shape.h).  Without a device the
driver checks that the reference's two errors (Filterbank.C:199-205) are thrown and that the base engine refuses a matrix
response, and stops with exit code 77; on a GPU an ndim 8 response must reach the matrix entry point and an ndim 2 response the
scalar one, each bit-identical to the C-ABI driven directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_driver(tmp_path):
    exe = tmp_path / "matrix_adaptor_driver"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "tests", "host_mock"),
           "-I", os.path.join(ROOT, "dspsr_amd", "host"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "matrix_adaptor_driver.cpp"), "-o", str(exe),
           "-L", os.path.join(ROOT, "dspsr_amd"), "-ldspsr_amd", "-Wl,-rpath," + os.path.join(ROOT, "dspsr_amd")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def test_matrix_adaptor_compiles_and_throws_the_reference_errors(tmp_path):
    import torch
    exe = _build_driver(tmp_path)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert "host engine ok" in p.stdout, p.stdout + p.stderr
    if torch.cuda.is_available():
        assert p.returncode == 0, p.stdout + p.stderr
    else:
        assert p.returncode == 77 and "no HIP device" in p.stdout


@pytest.mark.gpu
def test_matrix_adaptor_reaches_both_entry_points(tmp_path):
    exe = _build_driver(tmp_path)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ndim 8: matrix entry point" in p.stdout and "ndim 2: scalar entry point" in p.stdout
    assert "matrix adaptor driver ok" in p.stdout
