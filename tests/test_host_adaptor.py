"""The C++ adaptor header (dspsr_amd/host/dspsr_amd_engines.h) that binds the C-ABI to dsp::Filterbank::Engine /
dsp::Convolution::Engine / dsp::Detection::Engine / dsp::Fold::Engine / dsp::Memory / dsp::TimeSeries::Engine.

tests/host_adaptor_driver.cpp is built against the functional miniatures of tests/host_mock (the reference's interfaces
restated, virtual signatures as declared there) and run; on a GPU (`-m gpu`) it drives the adaptors in the reference's call
order -- Filterbank setup/perform, Detection in place, Fold prepare_output -> set_nbin -> set_ndat -> set_bins -> fold ->
synch -> zero -- and checks the sums bit for bit against the CPU loop of Fold.C:835-891; without a device it must stop
cleanly (exit code 77).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_driver(tmp_path):
    exe = tmp_path / "host_adaptor_driver"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "tests", "host_mock"),
           "-I", os.path.join(ROOT, "dspsr_amd", "host"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host_adaptor_driver.cpp"), "-o", str(exe),
           "-L", os.path.join(ROOT, "dspsr_amd"), "-ldspsr_amd", "-Wl,-rpath," + os.path.join(ROOT, "dspsr_amd")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def test_adaptor_driver_builds_and_stops_cleanly_without_a_device(tmp_path):
    import torch
    exe = _build_driver(tmp_path)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert p.returncode == 0, p.stdout + p.stderr
    else:
        assert p.returncode == 77 and "no HIP device" in p.stdout     # no CPU path: the context cannot be created


@pytest.mark.gpu
def test_adaptors_run_in_the_reference_call_order(tmp_path):
    exe = _build_driver(tmp_path)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "host adaptor driver ok" in p.stdout
