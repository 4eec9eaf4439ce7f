"""The calls the search-mode drivers (LoadToFil, LoadToFilCoherent, LoadToFilDirect, LoadToFITS) make on the device, call by call, on
the host: the engines, the context, the device allocator and every device operation dspsr_amd.pipeline calls are replaced by
recording fakes that return the host arithmetic of the real ones, four calls run through process_block, and the recorded trace of
every case is compared with a fixture under tests/golden/search_trace/ (the method, and the machinery, of
test_pipeline_trace_host).  A tensor is recorded by shape, strides, storage offset and the shape of the allocation it views: the
fixture shows which buffer a call writes without depending on the order of allocations.  The fixtures pin the block-to-block logic
-- carried tails, block collection, which operation runs on which part of which buffer -- through a restructuring of the drivers:
the test reads only the public surface of an instance.

    python tests/test_search_trace_host.py --regenerate

rewrites the fixtures from the code as it stands (nothing else does: not the environment, not a pytest option)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from dspsr_amd import pipeline                                                       # noqa: E402
from test_pipeline_trace_host import Log, _enc, recorded                            # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_trace")


class SearchLog(Log):
    """Tensors by shape, strides, offset and the shape of the allocation they view (None: not one of the driver's, the raw block)."""

    def __init__(self):
        super().__init__()
        self.allocations, self.used, self.built, self.kept = {}, set(), [], []

    def allocate(self, shape, dtype):
        t = torch.zeros(shape, dtype=getattr(torch, dtype))
        self.allocations[t.untyped_storage().data_ptr()] = list(t.shape)
        self.kept.append(t)                              # (alive for the run: no address is given out twice)
        return t

    def tensor(self, v):
        ptr = v.untyped_storage().data_ptr()
        self.used.add(ptr)
        return {"tensor": list(v.shape), "strides": list(v.stride()), "offset": v.storage_offset(), "of": self.allocations.get(ptr)}

    def open(self, obj, *a, **k):
        self.opened.append(obj)
        self.built.append([self.name(obj), [_enc(self, x) for x in a], {key: _enc(self, k[key]) for key in sorted(k)}])


def _fakes(mp):
    """Engines and operations that record every call and return what the real ones would, as far as the host logic reads it."""
    log = SearchLog()

    class Fake:
        def __init__(self, *a, **k):
            log.open(self, *[x for x in a if not isinstance(x, Context)], **k)

        def close(self):
            pass

        def synchronize(self):
            pass

    class Context(Fake):
        def __init__(self, device=0, stream=None):
            super().__init__()
            self.device, self.handle = device, 1

    class Filterbank(Fake):
        def setup(self, nsub, ndat, pos, neg, in_nchan, npol, real, kernel, **k):
            """the geometry the real engine derives: ndat - pos - neg samples kept per part of nsub * ndat (real: twice) input samples"""
            per = nsub * (2 if real else 1)
            self.nkeep, self.nsamp_step, self.nsamp_overlap, self.nsamp_fft = ndat - pos - neg, (ndat - pos - neg) * per, (pos + neg) * per, ndat * per
            log.call(self, "setup", nsub, ndat, pos, neg, in_nchan, npol, real, None if kernel is None else np.asarray(kernel).shape, **k)
            return self

        def search_is_fused(self):
            return True

        def set_guppi(self, *geometry):
            log.call(self, "set_guppi", *geometry)

        def perform_search(self, out, carry, carry_count, npart, tscrunch, state, **k):
            log.call(self, "perform_search", out, carry, carry_count, npart, tscrunch, state, **k)
            return divmod(carry_count + npart * self.nkeep, tscrunch)

        def perform_detect(self, det, npart, state, ndim, **k):
            log.call(self, "perform_detect", det, npart, state, ndim, **k)

    class Delay(Fake):
        def __init__(self, ctx, delays, npol=1, absolute=False):
            super().__init__(delays, npol)
            d = np.asarray(delays, np.int64)
            self.zero_delay = int(d.max())
            self.total_delay = int((self.zero_delay - d).max())

        def transform(self, inp, out=None):
            log.call(self, "transform", inp, out)
            return max(0, inp.shape[2] - self.total_delay)

    @recorded(log, "transform", "transform_fpt", "digitize_fpt", "pscrunch_digitize")
    class Rescale(Fake):
        pass

    class Digitizer(Fake):
        def __init__(self, ctx, nchan, npol, nbit, nsblk, *a, **k):
            super().__init__(nchan, npol, nbit, nsblk, *a, **k)
            self.block_bytes = nsblk * npol * nchan * nbit // 8

        def pack(self, inp, out, dat_scl, dat_offs):
            log.call(self, "pack", inp, out, dat_scl, dat_offs)

    def op(name, returns=lambda *a, **k: None):
        def fn(ctx, *a, **k):
            log.call("pipeline", name, *a, **k)
            return returns(*a, **k)
        mp.setattr(pipeline, name, fn)

    for name, cls in (("Context", Context), ("FilterbankEngine", Filterbank), ("SampleDelay", Delay), ("Rescale", Rescale),
                      ("FITSDigitizer", Digitizer)):
        mp.setattr(pipeline, name, cls)
    mp.setattr(pipeline, "_device_empty", lambda ctx, shape, dtype="float32", zero=False: log.allocate(shape, dtype))
    for name in ("tfp_filterbank", "pscrunch_tfp", "sigproc_digitize", "sigproc_digitize_fpt", "copy_data_fpt", "move_tail_fpt"):
        op(name)
    op("fscrunch_fpt", lambda inp, out, sfactor: out)
    op("tscrunch_fpt", lambda inp, out, sfactor, carry, carry_count=0, ndim=1: divmod(carry_count + inp.shape[2] // ndim, sfactor))
    op("detect_raw", lambda raw, out, carry, carry_count, nchan, npol, tscrunch=1, state=0, scale=1.0, ndat=None:
       divmod((carry_count or 0) + ndat, tscrunch))
    return log


# 8-bit real dual-polarisation input at 800 MHz (test_gpu_search); 8 complex channels of 1 MHz (test_gpu_direct_search); four
# MeerKAT channels of 4 MHz in heaps, and the two inputs of test_gpu_fits_pipeline
REAL = dict(centre_frequency=1382.0, bandwidth=-400.0, nchan=1, npol=2, ndim=1, tsamp_us=0.00125, machine="DADA")
CHANS = dict(centre_frequency=1400.0, bandwidth=-8.0, nchan=8, npol=2, ndim=2, tsamp_us=1.0, machine="DADA", start_seconds=0.5,
             mjd_day=55299, mjd_sec=7545.0)
HEAPS = dict(centre_frequency=1382.0, bandwidth=-16.0, nchan=4, npol=2, ndim=2, tsamp_us=0.25, machine="MKBFRo")
GUPPI = dict(HEAPS, machine="GUPPI", guppi=(200, 832, 3328))          # (8 samples of every run overlap the next block)
FITS_REAL = dict(centre_frequency=1400.0, bandwidth=-16.0, nchan=1, npol=2, ndim=1, tsamp_us=1.0 / 32.0, machine="DADA")
FITS_CHANS = dict(centre_frequency=1400.0, bandwidth=4.0, nchan=4, npol=2, ndim=2, tsamp_us=1.0, machine="DADA", source="J0000+0000")
TFP = dict(nchan=64, tscrunch=16, nbit=8, rescale_seconds=2e-4, parts_per_block=64)
COHERENT = dict(nchan=64, tscrunch=16, nbit=8, rescale_seconds=2e-4, freq_res=1024, parts_per_block=3, max_parts=4)
DIRECT = dict(tscrunch=4, nbit=8, rescale_seconds=256.5 * 4 / 1e6, parts_per_block=64)


def _search(cls, info, **cfg):
    return lambda: getattr(pipeline, cls)(pipeline.SearchConfig(**cfg), pipeline.InputInfo(**info))


def _fits(info, **cfg):
    return lambda: pipeline.LoadToFITS(pipeline.FitsConfig(nsblk=128, **cfg), pipeline.InputInfo(**info))


# name -> (driver, the count of each of the four calls: parts, or time samples with no -F; the last call is ragged)
CASES = {
    "fil_fused": (_search("LoadToFil", REAL, **TFP), (64, 64, 64, 32)),
    "fil_float": (_search("LoadToFil", REAL, **{**TFP, "nbit": -32}), (64, 64, 64, 32)),
    "coherent_fused": (_search("LoadToFilCoherent", REAL, dispersion_measure=2.0, **COHERENT), (3, 3, 3, 2)),
    # -K -f 4 with no Rescale: the digitiser divides by input_scale
    "coherent_K_f": (_search("LoadToFilCoherent", REAL, dispersion_measure=0.25, dedisperse=True, fscrunch=4,
                             **{**COHERENT, "rescale_seconds": 0.0}), (3, 3, 3, 2)),
    # -d 4 on heaps: blocks of 3 parts of 462 samples begin at samples 0, 106, 212, 62 of their first heaps
    "coherent_d4_heaps": (_search("LoadToFilCoherent", HEAPS, nchan=4, dispersion_measure=10.0, freq_res=1024, tscrunch=4, npol=4, nbit=8,
                                  rescale_seconds=0.0, parts_per_block=3, max_parts=2), (3, 3, 3, 2)),
    # the same channels as GUPPI raw blocks of 200 kept samples per run: the blocks begin at samples 0, 186, 172, 158 of their first one
    "coherent_guppi": (_search("LoadToFilCoherent", GUPPI, nchan=4, dispersion_measure=10.0, freq_res=1024, tscrunch=4, npol=2, nbit=8,
                               rescale_seconds=0.0, parts_per_block=3, max_parts=2), (3, 3, 3, 2)),
    "fits_F_guppi": (_fits(GUPPI, nchan=4, convolve=True, dispersion_measure=10.0, coherent_dedisp=True, tsamp=16e-6,
                           parts_per_block=3, npol=2, nbit=8), (3, 3, 3, 2)),
    "direct_fused": (_search("LoadToFilDirect", CHANS, **DIRECT), (64, 64, 64, 30)),
    "direct_K_f": (_search("LoadToFilDirect", CHANS, dispersion_measure=2.0, dedisperse=True, fscrunch=2, npol=2, **DIRECT), (64, 64, 64, 30)),
    "direct_K_empty_call": (_search("LoadToFilDirect", CHANS, dispersion_measure=2.0, dedisperse=True, **{**DIRECT, "nbit": -32, "rescale_seconds": 0.0}),
                            (64, 0, 64, 30)),
    # the cuts of test_gpu_fits_pipeline: 127.75 scrunched samples per part, 128 per block
    "fits_F_D": (_fits(FITS_REAL, nchan=16, convolve=True, freq_res=256, dispersion_measure=1.0, coherent_dedisp=True, tsamp=16e-6,
                       parts_per_block=14, nbit=8), (1, 5, 2, 6)),
    "fits_F_K": (_fits(FITS_REAL, nchan=16, freq_res=256, dispersion_measure=30.0, dedisperse=True, tsamp=16e-6, parts_per_block=14, npol=1,
                       nbit=4, rescale_seconds=0.004), (1, 5, 2, 6)),
    "fits_direct_K": (_fits(FITS_CHANS, nchan=0, dispersion_measure=100.0, dedisperse=True, tsamp=16e-6, parts_per_block=8192, npol=2, nbit=2),
                      (100, 7000, 0, 5887)),
}


def _first_sample(drv, k, counts):
    """where in its first heap, or in the runs of its first GUPPI raw block, call k begins (zero for every other input), as the
    readers' blocks() count it"""
    if drv.info.machine != "MKBFRo" and drv.info.guppi is None:
        return 0
    return (sum(counts[:k]) * drv.front.nsamp_step) % (256 if drv.info.guppi is None else drv.info.guppi[0])


def _run(mp, name):
    """Four calls of case `name`: the engines opened, the calls, the returns and the counters, as the fixture holds them."""
    log = _fakes(mp)
    build, counts = CASES[name]
    drv = build()
    fits = isinstance(drv, pipeline.LoadToFITS)
    opened, marks, returned, counters = list(log.built), [], [], []
    for k, n in enumerate(counts):
        marks.append(len(log.calls))
        first = _first_sample(drv, k, counts)
        args = (n, first) if first else (n,)
        raw = torch.zeros(drv.block_bytes(*args), dtype=torch.int8)
        out = drv.process_block(raw, *args)
        returned.append(len(out) if fits else log.tensor(out))
        names = ("fill", "nblocks_out") if fits else ("ndat_out", "carry_count", "sd_carried")
        counters.append({c: getattr(drv, c, None) for c in names})
    marks.append(len(log.calls))
    result = {"opened": opened, "setup": log.calls[:marks[0]], "blocks": [log.calls[a:b] for a, b in zip(marks, marks[1:])],
              "returned": returned, "counters": counters, "header": {k: _enc(log, v) for k, v in drv.header_values().items()}}
    drv.close()
    return json.loads(json.dumps(result)), log


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_trace_of_four_calls_is_the_recorded_one(monkeypatch, name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        want = json.load(f)
    got, _ = _run(monkeypatch, name)
    assert got["opened"] == want["opened"] and got["setup"] == want["setup"]
    for k, (g, w) in enumerate(zip(got["blocks"], want["blocks"])):
        for i, (cg, cw) in enumerate(zip(g, w)):
            assert cg == cw, "call %d, operation %d" % (k, i)
        assert len(g) == len(w), "call %d" % k
    for key in ("returned", "counters", "header"):
        assert got[key] == want[key], key
    assert sorted(got) == sorted(want)


def _fixture(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def _methods(block):
    return [c[1] for c in block]


def test_the_blocks_chosen_reach_the_branches():
    """what the fixtures are worth, from the fixtures themselves: each branch of the four drivers occurs in one of them"""
    # LoadToFil: the one-pass output stage; with -b -32 Rescale, PScrunch and the digitiser one after the other
    assert all(_methods(b) == ["tfp_filterbank", "pscrunch_digitize"] for b in _fixture("fil_fused")["blocks"])
    assert all(_methods(b) == ["tfp_filterbank", "transform", "pscrunch_tfp", "sigproc_digitize"] for b in _fixture("fil_float")["blocks"])
    # LoadToFilCoherent: fused; -K -f 4 unfused with a tail carried over every block and no Rescale; -d 4 on heaps
    fused = _fixture("coherent_fused")
    assert all(_methods(b) == ["perform_search", "digitize_fpt"] for b in fused["blocks"]) and fused["blocks"][0][0][2][4] == 16
    kf = _fixture("coherent_K_f")
    assert all(_methods(b)[:4] == ["perform_search", "transform", "fscrunch_fpt", "tscrunch_fpt"] and "move_tail_fpt" in _methods(b)
               and _methods(b)[-1] == "sigproc_digitize_fpt" for b in kf["blocks"])
    assert all(c["sd_carried"] > 0 for c in kf["counters"]) and kf["blocks"][0][0][2][4] == 1
    assert all(b[-1][3]["input_scale"] != repr(1.0) and b[-1][3]["use_digi_scales"] is False for b in kf["blocks"])
    d4 = _fixture("coherent_d4_heaps")
    assert all(_methods(b)[:2] == ["perform_detect", "tscrunch_fpt"] for b in d4["blocks"])
    layouts = [b[0][3]["layout"] for b in d4["blocks"]]
    assert len(set(layouts)) > 1, "a block that begins inside a heap"
    # GUPPI raw blocks: the geometry goes to the engine once, every call carries the layout word of its own first sample
    for name in ("coherent_guppi", "fits_F_guppi"):
        fx = _fixture(name)
        assert fx["setup"][-1][1:3] == ["set_guppi", [200, 832, 3328]], name
        words = [b[0][3]["layout"] for b in fx["blocks"]]
        assert all(w & 0xff == 6 for w in words) and words[0] == 6 and len(set(words)) == 4, (name, words)
    # LoadToFilDirect: one pass; -K -f; an empty call between two others does nothing but carry the tail along
    assert all(_methods(b) == ["detect_raw", "digitize_fpt"] for b in _fixture("direct_fused")["blocks"])
    dkf = _fixture("direct_K_f")
    assert all(_methods(b)[:4] == ["detect_raw", "transform", "fscrunch_fpt", "tscrunch_fpt"] for b in dkf["blocks"])
    assert all(c["sd_carried"] > 0 for c in dkf["counters"])
    empty = _fixture("direct_K_empty_call")
    assert empty["returned"][1]["tensor"] == [0] and "tscrunch_fpt" not in _methods(empty["blocks"][1])
    assert empty["blocks"][1][0][3]["ndat"] == 0 and empty["counters"][1] == empty["counters"][0]
    assert "tscrunch_fpt" in _methods(empty["blocks"][2])
    # LoadToFITS: a call that completes no block, one that completes at least two, the remainder moved to the front
    for name in ("fits_F_D", "fits_direct_K"):
        fx = _fixture(name)
        assert 0 in fx["returned"] and max(fx["returned"]) >= 2, (name, fx["returned"])
        assert any("move_tail_fpt" in _methods(b) and "pack" in _methods(b) for b in fx["blocks"]), name
        assert [_methods(b).count("pack") for b in fx["blocks"]] == fx["returned"]
    assert "perform_detect" in _methods(_fixture("fits_F_D")["blocks"][0])                 # -p 4: the unfused branch of the front end
    for name in ("fits_F_K", "fits_direct_K"):                                              # -K at the scrunched rate
        fx = _fixture(name)
        assert any(_methods(b).count("transform") == 1 and "copy_data_fpt" in _methods(b) for b in fx["blocks"]), name
    assert "perform_search" in _methods(_fixture("fits_F_K")["blocks"][0]) and "detect_raw" in _methods(_fixture("fits_direct_K")["blocks"][0])
    assert sum(_fixture("fits_F_K")["returned"]) >= 1


def test_every_buffer_load_to_fits_allocates_is_used(monkeypatch):
    """every allocation of a LoadToFITS is passed to at least one recorded call of its four: none is made to be left alone"""
    for name in ("fits_F_D", "fits_F_K", "fits_direct_K"):
        _, log = _run(monkeypatch, name)
        unused = [shape for ptr, shape in log.allocations.items() if ptr not in log.used]
        assert log.allocations and unused == [], (name, unused)


def regenerate():
    os.makedirs(GOLDEN, exist_ok=True)
    for name in sorted(CASES):
        with pytest.MonkeyPatch.context() as mp:
            result, _ = _run(mp, name)
        with open(os.path.join(GOLDEN, name + ".json"), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print("%s: %d calls, returned %s" % (name, sum(len(b) for b in result["blocks"]), [r if isinstance(r, int) else r["tensor"] for r in result["returned"]]))


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_search_trace_host.py --regenerate")
    regenerate()
