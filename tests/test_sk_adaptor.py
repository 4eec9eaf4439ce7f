"""HIP::SpectralKurtosisEngine (dspsr_amd/host/dspsr_amd_sk_engine.h), the adaptor that binds the spectral-kurtosis object to
dsp::SpectralKurtosis::Engine.  tests/sk_adaptor_driver.cpp is built against the miniatures of tests/host_mock
(dsp/SpectralKurtosis.h: the reference's virtual signatures and call order) and run.  Without a device it runs the miniature's CPU
engine, checks that the adaptor refuses a null context, and stops with exit code 77; on a GPU it drives the adaptor in the
reference's call order and requires estimates, mask, cleaned rows and counters bit-identical to the CPU engine and to the C-ABI path."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_driver(tmp_path):
    exe = tmp_path / "sk_adaptor_driver"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "tests", "host_mock"),
           "-I", os.path.join(ROOT, "dspsr_amd", "host"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sk_adaptor_driver.cpp"), "-o", str(exe),
           "-L", os.path.join(ROOT, "dspsr_amd"), "-ldspsr_amd", "-Wl,-rpath," + os.path.join(ROOT, "dspsr_amd")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def test_sk_adaptor_compiles_and_instantiates(tmp_path):
    import torch
    exe = _build_driver(tmp_path)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert "host engine ok" in p.stdout, p.stdout + p.stderr
    if torch.cuda.is_available():
        assert p.returncode == 0, p.stdout + p.stderr
    else:
        assert p.returncode == 77 and "no HIP device" in p.stdout


@pytest.mark.gpu
def test_sk_adaptor_runs_in_the_reference_call_order(tmp_path):
    exe = _build_driver(tmp_path)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sk adaptor driver ok" in p.stdout
