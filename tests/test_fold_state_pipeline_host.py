"""`-d 1`, `-d 2` and one-polarisation input on the plain path of pipeline.LoadToFold, and the tool's options, without a device:
the host plan alone (LoadToFold._plan opens nothing), what it refuses by name, and the hand-off file's header."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pipeline():
    from dspsr_amd import pipeline
    return pipeline


def _planned(cfg, info, **kw):
    pipeline = _pipeline()
    lt = object.__new__(pipeline.LoadToFold)
    lt._defaults()
    lt._plan(cfg, info, None, 0.0, kw.get("subband"), tuple(kw.get("dump_before", ())), list(kw.get("targets", [])))
    return lt


def _cfg(**kw):
    return _pipeline().Config(**{**dict(nchan=16, dispersion_measure=30.0, nbin=64, folding_period=0.004), **kw})


def _info(**kw):
    return _pipeline().InputInfo(**{**dict(centre_frequency=1382.0, bandwidth=-16.0, tsamp_us=1.0 / 32.0, machine="DADA"), **kw})


def test_npol_chooses_the_state_and_the_shapes():
    from dspsr_amd import _lib
    for npol, name, state, npo in ((1, "Intensity", _lib.INTENSITY, 1), (2, "PPQQ", _lib.PPQQ, 2)):
        for ndim in (4, 2, 1):                                       # the layout of the four products does not matter
            lt = _planned(_cfg(npol=npol, ndim=ndim), _info())
            assert lt.square_law == (name, state, npo) and lt.npol_out == npo and lt._fold_dims() == (npo, 1) and lt.cfg.ndim == 1
            assert lt.detection_state() == state and lt.state_name() == name
    lt = _planned(_cfg(ndim=2), _info())                             # npol 4: today's path
    assert lt.square_law is None and lt.npol_out == 2 and lt._fold_dims() == (2, 2) and lt.state_name() == "Coherence"
    assert _planned(_cfg(stokes=True), _info()).state_name() == "Stokes"


def test_npol_3_is_the_references_refusal():
    from dspsr_amd import DspsrAmdError
    with pytest.raises(DspsrAmdError, match="dsp::Detection cannot convert from Analytic to NthPower"):
        _planned(_cfg(npol=3), _info())
    with pytest.raises(DspsrAmdError, match="dsp::Detection cannot convert from Analytic to NthPower"):
        _planned(_cfg(npol=3, fourth_moment=True), _info())          # -4 loses to npol 3
    with pytest.raises(DspsrAmdError, match="npol=5 is not one of"):
        _planned(_cfg(npol=5), _info())


def test_fourth_moment_loses_to_npol_1_and_wins_over_2():
    lt = _planned(_cfg(npol=1, fourth_moment=True), _info())
    assert not lt.moments and lt.square_law[0] == "Intensity" and lt._fold_dims() == (1, 1)
    lt = _planned(_cfg(npol=2, fourth_moment=True), _info())
    assert lt.moments and lt.square_law is None and lt._fold_dims() == (1, 14) and lt.state_name() == "FourthMoment"


def test_one_polarisation_plans_pp(capsys):
    from dspsr_amd import DspsrAmdError, _lib
    for npol in (1, 2, 3):
        lt = _planned(_cfg(npol=npol), _info(npol=1, ndim=2))
        assert lt.square_law == ("PP", _lib.INTENSITY, 1) and lt._fold_dims() == (1, 1) and lt.state_name() == "PP"
        assert "Only single polarization detection available" in capsys.readouterr().err
    # the default npol = 4 keeps the refusal this path has always had
    with pytest.raises(DspsrAmdError, match="Cannot detect polarization when npol != 2"):
        _planned(_cfg(), _info(npol=1, ndim=2))


@pytest.mark.parametrize("npol", [1, 2])
def test_refused_combinations_are_named(npol):
    from dspsr_amd import DspsrAmdError
    cases = [(dict(sk_zap=True), {}, r"npol=%d \(-d %d\) is not built with spectral kurtosis \(-skz\)" % (npol, npol)),
             (dict(calibrator=(np.array([1382.0]), np.eye(2)[None])), {}, r"is not built with the calibrator \(-pac\)"),
             (dict(convolve_when="after"), {}, r"is not built with convolve_when='after'"),
             (dict(convolve_when="before"), {}, r"is not built with convolve_when='before'"),
             (dict(convolve_when="never"), {}, r"is not built with convolve_when='never'")]
    for ckw, ikw, text in cases:
        with pytest.raises(DspsrAmdError, match=text):
            _planned(_cfg(npol=npol, **ckw), _info(**ikw))
    with pytest.raises(DspsrAmdError, match=r"two-bit input \(NBIT 2\)"):
        _planned(_cfg(npol=npol, nchan=8), _info(nbit=2, machine="CPSR2", ndim=1))
    # -cyclic and -G keep their own reading of npol
    assert _planned(_cfg(npol=npol, plfb_nbin=8, nbin=8, ndim=1), _info()).square_law is None
    assert _planned(_cfg(npol=npol, cyclic_nchan=16, cyclic_npol=npol, nbin=32), _info()).square_law is None


def test_shape_agnostic_combinations_plan():
    pipeline = _pipeline()
    lt = _planned(_cfg(npol=2, subint_seconds=0.002), _info())
    assert lt.square_law[0] == "PPQQ"
    lt = _planned(_cfg(npol=1, interchan_dedispersion=True, dispersion_measure=1.0), _info())
    assert lt.square_law[0] == "Intensity" and lt._delays is not None
    lt = _planned(_cfg(npol=2), _info(), dump_before=("Fold",))
    assert lt._taps == ("Fold",)
    targets = [pipeline.FoldTarget("a", folding_period=0.004, nbin=64), pipeline.FoldTarget("b", folding_period=0.005, nbin=32)]
    assert _planned(_cfg(npol=2), _info(), targets=targets).npol_out == 2


def test_hand_off_file_carries_state_npol_ndim(tmp_path):
    pipeline = _pipeline()
    rng = np.random.default_rng(2)
    hits = rng.integers(1, 99, 37).astype(np.uint32)
    for npol, info, want in ((1, _info(), ("Intensity", 1, 1)), (2, _info(), ("PPQQ", 2, 1)), (2, _info(npol=1, ndim=2), ("PP", 1, 1))):
        npo = want[1]
        prof = rng.standard_normal((3, npo, 37, 1)).astype(np.float32)
        sub = {"hits": hits, "integration_length": 0.5, "ndat_total": int(hits.sum()), "profile": prof}
        path = str(tmp_path / "s.ps")
        pipeline.write_phase_series(path, sub, info, _cfg(nchan=3, nbin=37, npol=npol), npol=npo)
        hdr, h, p = pipeline.read_phase_series(path)
        assert (hdr["STATE"], int(hdr["NPOL"]), int(hdr["NDIM"])) == want and np.array_equal(p, prof) and np.array_equal(h, hits)


def _tool():
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool", os.path.join(ROOT, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_maps_d_and_ndim():
    tool = _tool()
    base = ["-F", "16:D", "-c", "0.004", "x.dada"]
    opt = lambda *extra: tool.detection_options(tool.parse_args(list(extra) + base))
    assert opt() == dict(ndim=4, npol=4, cyclic_npol=0)
    assert opt("-d", "1") == dict(ndim=4, npol=1, cyclic_npol=0)
    assert opt("-d", "2", "-ndim", "2") == dict(ndim=2, npol=2, cyclic_npol=0)
    assert opt("-ndim", "1") == dict(ndim=1, npol=4, cyclic_npol=0)                 # the layout -d spelled before
    assert opt("-d", "3") == dict(ndim=4, npol=3, cyclic_npol=0)                 # LoadToFold reports the reference's error
    # -cyclic and -G: nothing changed
    assert opt("-cyclic", "16", "-d", "2") == dict(ndim=1, npol=4, cyclic_npol=2)
    assert tool.detection_options(tool.parse_args(["-cyclic", "16", "-d", "2"] + base), input_npol=1) == dict(ndim=1, npol=4, cyclic_npol=1)
    assert opt("-G", "8", "-d", "2") == dict(ndim=1, npol=2, cyclic_npol=0)
    assert opt("-G", "8") == dict(ndim=1, npol=4, cyclic_npol=0)
    with pytest.raises(SystemExit):
        tool.parse_args(["-d", "5"] + base)
    for mode in (["-cyclic", "16"], ["-G", "8"]):                                  # -d 3 is the plain path's alone
        with pytest.raises(SystemExit):
            tool.parse_args(mode + ["-d", "3"] + base)
    with pytest.raises(SystemExit):                                               # no -n: -noskz_too stays an unrecognised argument
        tool.parse_args(["-noskz_too"] + base)
    from dspsr_amd import DspsrAmdError
    cfg = dataclasses.replace(_cfg(), **opt("-d", "3"))
    with pytest.raises(DspsrAmdError, match="NthPower"):
        _planned(cfg, _info())
