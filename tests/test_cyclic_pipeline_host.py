"""The cyclic-spectrum route of LoadToFold without a device: what it refuses (before any device resource is opened), the shape
and state of its output, the tool's options and the hand-off file."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

from dspsr_amd import DspsrAmdError, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = pipeline.Config(nchan=16, dispersion_measure=30.0, nbin=64, folding_period=0.004, cyclic_nchan=32)
INFO = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=-16.0, npol=2, ndim=1, tsamp_us=1.0 / 32.0, machine="DADA")


@pytest.mark.parametrize("change,kwargs,text", [
    (dict(subint_turns=1.0), {}, "Single-pulse and cyclic spectrum modes are incompatible"),
    (dict(interchan_dedispersion=True), {}, "-K"),
    (dict(convolve_when="after"), {}, "convolve_when"),
    (dict(convolve_when="before"), {}, "convolve_when"),
    (dict(convolve_when="never"), {}, "convolve_when"),
    ({}, dict(subband=0), "sub-band"),
    ({}, dict(dump_before=("Fold",)), "dump"),
    ({}, dict(targets=[pipeline.FoldTarget(folding_period=0.004), pipeline.FoldTarget(folding_period=0.005)]), "one pulsar"),
    (dict(cyclic_npol=3), {}, "invalid npol"),
    (dict(cyclic_nchan=24), {}, "powers of two"),
    (dict(cyclic_nchan=3), {}, "even"),
])
def test_cyclic_refusals_at_construction(change, kwargs, text):
    with pytest.raises(DspsrAmdError, match=text):
        pipeline.LoadToFold(dataclasses.replace(CFG, **change), INFO, **kwargs)


def test_one_polarisation_gives_npol_one_only():
    one = dataclasses.replace(INFO, npol=1)
    with pytest.raises(DspsrAmdError, match="one input polarisation"):
        pipeline.LoadToFold(dataclasses.replace(CFG, cyclic_npol=4), one)
    g = pipeline.cyclic_geometry(CFG, one)
    assert (g["npol"], g["state"]) == (1, "PP")


@pytest.mark.parametrize("n,m,npol,state", [(32, 1, 0, "Coherence"), (32, 4, 2, "PPQQ"), (1024, 4, 1, "Intensity"), (256, 1, 4, "Coherence")])
def test_cyclic_geometry(n, m, npol, state):
    g = pipeline.cyclic_geometry(dataclasses.replace(CFG, cyclic_nchan=n, cyclic_mover=m, cyclic_npol=npol), INFO)
    assert g["nlag"] == m * n // 2 + 1 and g["nchan_spec"] == 2 * g["nlag"] - 2 == m * n
    assert g["nchan_per_channel"] == n and g["nchan"] == CFG.nchan * n
    assert g["ndim"] == 1 and g["npol"] == (npol or 4) and g["state"] == state


def test_cyclic_off_is_the_default():
    c = pipeline.Config()
    assert (c.cyclic_nchan, c.cyclic_mover, c.cyclic_npol) == (0, 1, 0)


def test_cyclic_subint_file_round_trip(tmp_path):
    g = pipeline.cyclic_geometry(dataclasses.replace(CFG, cyclic_npol=2), INFO)
    rng = np.random.default_rng(3)
    spectra = rng.standard_normal((g["nchan"], g["npol"], CFG.nbin)).astype(np.float32)
    sub = {"hits": rng.integers(1, 9, CFG.nbin).astype(np.uint32), "integration_length": 0.25, "ndat_total": 1234,
           "profile": spectra[..., None]}
    path = str(tmp_path / "c.ps")
    pipeline.write_phase_series(path, sub, INFO, dataclasses.replace(CFG, ndim=1), nchan=g["nchan"], npol=g["npol"], state=g["state"])
    hdr, hits, prof = pipeline.read_phase_series(path)
    assert (int(hdr["NCHAN"]), int(hdr["NPOL"]), int(hdr["NDIM"]), hdr["STATE"]) == (16 * 32, 2, 1, "PPQQ")
    assert np.array_equal(hits, sub["hits"]) and np.array_equal(prof[..., 0], spectra)


def test_tool_options():
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool_cyclic", os.path.join(ROOT, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["-F", "64:D", "-cyclic", "256", "-cyclicoversample", "4", "-c", "0.004", "x.dada"])
    assert (a.cyclic, a.cyclic_mover) == (256, 4)
    a = tool.parse_args(["-F", "64:D", "-c", "0.004", "x.dada"])
    assert (a.cyclic, a.cyclic_mover, a.ndim) == (0, 1, 4)
