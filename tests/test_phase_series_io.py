"""SURVEY 8f-3, reader side: the PhaseSeries hand-off file written by pipeline.write_phase_series is read back by the C++
reader a DSPSR maintainer would call before Archiver::unload (dspsr_amd/host/dspsr_amd_phase_series_io.h): the plain-C++
layer is compiled and run here on a file written by the product (checksums must agree)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
#include "dspsr_amd_phase_series_io.h"
int main (int argc, char** argv)
{
  try {
    HIP::PhaseSeriesFile f = HIP::read_phase_series_file (argv[1]);
    double s = 0; unsigned long long h = 0;
    for (size_t i = 0; i < f.sums.size (); i++) s += double (f.sums[i]) * double (i % 7 + 1);
    for (size_t i = 0; i < f.hits.size (); i++) h += (unsigned long long) f.hits[i] * (i + 1);
    printf ("%u %u %u %u %.17g %llu %.17g %s %.17g\n", f.nchan, f.npol, f.ndim, f.nbin, s, h, f.number ("INTEGRATION_LENGTH"),
            f.text ("STATE").c_str (), f.number ("SCALE"));
  } catch (std::exception& e) { fprintf (stderr, "%s\n", e.what ()); return 1; }
  return 0;
}
'''


def test_reader_reads_what_the_product_writes(tmp_path):
    from dspsr_amd import pipeline
    rng = np.random.default_rng(3)
    nchan, npol, nbin, ndim = 6, 2, 32, 2
    sub = {"hits": rng.integers(0, 1000, nbin).astype(np.uint32), "integration_length": 12.625, "ndat_total": 4931712,
           "profile": rng.standard_normal((nchan, npol, nbin, ndim)).astype(np.float32)}
    info = pipeline.InputInfo()
    cfg = pipeline.Config(nchan=nchan, nbin=nbin, ndim=ndim, stokes=True, folding_period=0.0893)
    path = str(tmp_path / "sub0.ps")
    pipeline.write_phase_series(path, sub, info, cfg, npol=npol, scale=1.7179869184e10, division=3, folding_period=0.0893)
    src = tmp_path / "r.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "r"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "dspsr_amd", "host"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), path], check=True, capture_output=True, text=True).stdout.split()
    flat = sub["profile"].reshape(-1).astype(np.float64)
    want_s = float((flat * (np.arange(flat.size) % 7 + 1)).sum())
    want_h = int((sub["hits"].astype(np.int64) * (np.arange(nbin) + 1)).sum())
    assert [int(v) for v in out[:4]] == [nchan, npol, ndim, nbin]
    assert abs(float(out[4]) - want_s) <= 1e-9 * abs(want_s) and int(out[5]) == want_h
    assert float(out[6]) == 12.625 and out[7] == "Stokes" and float(out[8]) == 1.7179869184e10
    # and the Python reader of the same file agrees (pipeline.read_phase_series)
    hdr, hits, prof = pipeline.read_phase_series(path)
    assert np.array_equal(hits, sub["hits"]) and np.array_equal(prof, sub["profile"]) and hdr["DIVISION"] == "3"
    # a truncated file is an error, not garbage
    open(str(tmp_path / "bad.ps"), "wb").write(open(path, "rb").read()[:5000])
    assert subprocess.run([str(exe), str(tmp_path / "bad.ps")], capture_output=True).returncode == 1
