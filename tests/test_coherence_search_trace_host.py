"""The calls LoadToFilCoherent -d 4 and LoadToFITS -p 4 make with `fuse_coherence`, on the host, with the recording fakes of
tests/test_search_trace_host.py: every block is then ONE perform_search (state Coherence, the time-scrunch factor) followed by the
output stage the recorded trace has -- no perform_detect, no tscrunch_fpt.  With the default (False) the trace is the recorded one,
call for call: the option changes nothing for a caller who does not set it."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_search_trace_host as ts                                                  # noqa: E402
from dspsr_amd import _lib, pipeline                                                 # noqa: E402

# the two recorded -d 4 / -p 4 configurations (test_search_trace_host.CASES), rebuilt here with the option
D4_HEAPS = dict(nchan=4, dispersion_measure=10.0, freq_res=1024, tscrunch=4, npol=4, nbit=8, rescale_seconds=0.0, parts_per_block=3, max_parts=2)
FITS_F_D = dict(nchan=16, convolve=True, freq_res=256, dispersion_measure=1.0, coherent_dedisp=True, tsamp=16e-6, parts_per_block=14, nbit=8)
BUILD = {
    "coherent_d4_heaps": lambda **kw: ts._search("LoadToFilCoherent", ts.HEAPS, **D4_HEAPS, **kw),
    "fits_F_D": lambda **kw: ts._fits(ts.FITS_REAL, **FITS_F_D, **kw),
}


def _trace(monkeypatch, name, **kw):
    monkeypatch.setitem(ts.CASES, name, (BUILD[name](**kw), ts.CASES[name][1]))
    return ts._run(monkeypatch, name)[0]


@pytest.mark.parametrize("name", sorted(BUILD))
def test_the_default_is_the_recorded_trace(monkeypatch, name):
    assert _trace(monkeypatch, name) == ts._fixture(name)
    assert _trace(monkeypatch, name, fuse_coherence=False) == ts._fixture(name)


@pytest.mark.parametrize("name", sorted(BUILD))
def test_fuse_coherence_is_one_perform_search_per_block(monkeypatch, name):
    want, got = ts._fixture(name), _trace(monkeypatch, name, fuse_coherence=True)
    build, counts = BUILD[name], ts.CASES[name][1]
    assert len(got["blocks"]) == len(want["blocks"]) == len(counts)
    factor = 4 if name == "coherent_d4_heaps" else 16
    for k, (g, w) in enumerate(zip(got["blocks"], want["blocks"])):
        gm, wm = ts._methods(g), ts._methods(w)
        assert wm[:2] == ["perform_detect", "tscrunch_fpt"]
        assert gm[0] == "perform_search" and "perform_detect" not in gm and "tscrunch_fpt" not in gm
        # the output stage: the operations of the recorded block behind its first two
        assert gm[1:] == wm[2:], "call %d" % k
        args = g[0][2]                                  # out, carry, carry_count, npart, tscrunch, state
        assert args[3] == counts[k] and args[4] == factor and args[5] == _lib.COHERENCE
        assert args[0]["tensor"][1] == 4 and args[1]["tensor"][-1] == 4          # four rows per channel, [nchan][4] carries
        # the raw block, its layout and scale are what perform_detect was given
        assert g[0][3] == w[0][3]
        # ... and the carried count is what the unfused TScrunch carried
        if k:
            assert args[2] == got["counters"][k - 1].get("carry_count", args[2])
    # what the driver returns and its books do not depend on the route
    for key in ("returned", "counters", "header", "setup"):
        assert got[key] == want[key], key


def test_the_option_reaches_both_configurations():
    assert "fuse_coherence" in pipeline.FRONT_OPTIONS
    assert pipeline.SearchConfig().fuse_coherence is False and pipeline.FitsConfig().fuse_coherence is False
    info = pipeline.InputInfo(**ts.REAL)
    kw = dict(nchan=64, tscrunch=16, dispersion_measure=2.0, freq_res=1024, parts_per_block=3, fscrunch=0, max_parts=4, dedisperse=False)
    for npol, fuse, want in ((4, False, False), (4, True, True), (1, False, True), (2, True, True)):
        assert pipeline.ConvolvingFront(info, npol=npol, fused=True, fuse_coherence=fuse, **kw).fused is want
    # -K and -f keep the unfused chain, and fused=False switches every state off
    assert not pipeline.ConvolvingFront(info, npol=4, fused=True, fuse_coherence=True, **{**kw, "fscrunch": 4}).fused
    assert not pipeline.ConvolvingFront(info, npol=4, fused=True, fuse_coherence=True, **{**kw, "dedisperse": True}).fused
    assert not pipeline.ConvolvingFront(info, npol=4, fused=False, fuse_coherence=True, **kw).fused
