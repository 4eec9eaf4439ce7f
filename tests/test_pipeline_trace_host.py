"""The calls LoadToFold makes on its engines, block by block, on the host: every engine, the context, the device allocator, the
tail move and the profile view of dspsr_amd.pipeline are replaced by recording fakes (as test_pipeline_construction_host does for
construction), four blocks run through process_block and finish_subint, and the recorded trace of every mode is compared with a
fixture under tests/golden/pipeline_trace/.  The fixtures pin the host logic -- which engine is called, with which numbers, on
which part of which buffer, in which order -- through a restructuring of the driver: the test reads only the public surface of
an instance.

    python tests/test_pipeline_trace_host.py --regenerate

rewrites the fixtures from the code as it stands (nothing else does: not the environment, not a pytest option)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dspsr_amd import dada, pipeline                                                # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_trace")
PARTS = (3, 3, 3, 2)                           # four blocks of parts_per_block = 3 parts, the last one ragged


def _enc(log, v):
    """One argument of a recorded call: scalars as they are (floats by repr), tensors by shape and storage offset, host arrays by
    shape, type and -- the short ones: window starts and bins -- values, engines by their place in the order of opening."""
    if isinstance(v, torch.Tensor):
        return log.tensor(v)
    if isinstance(v, np.ndarray):
        d = {"array": list(v.shape), "dtype": str(v.dtype)}
        if v.size <= 16:
            d["values"] = [int(x) for x in v.reshape(-1)]
        return d
    if isinstance(v, (list, tuple)):
        return [_enc(log, x) for x in v]
    if isinstance(v, (bool, int, str)) or v is None:
        return v
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    if isinstance(v, np.integer):
        return int(v)
    if v in log.opened:
        return log.name(v)
    raise TypeError("unrecorded argument %r" % (v,))


class Log:
    def __init__(self):
        self.opened, self.calls = [], []

    def name(self, obj):
        return "%s#%d" % (type(obj).__name__, self.opened.index(obj))

    def tensor(self, v):
        return {"tensor": list(v.shape), "offset": v.storage_offset()}

    def call(self, who, method, *a, **k):
        self.calls.append([who if isinstance(who, str) else self.name(who), method, [_enc(self, x) for x in a],
                           {key: _enc(self, k[key]) for key in sorted(k)}])


def recorded(log, *names, returns=None):
    """Class decorator: the methods `names` write their call into `log` and return `returns`."""
    def deco(cls):
        for n in names:
            def method(self, *a, _n=n, **k):
                log.call(self, _n, *a, **k)
                return returns
            setattr(cls, n, method)
        return cls
    return deco


def _fakes(mp):
    """Engines that record every call and return what the real ones would, as far as the host logic reads it."""
    log = Log()

    class Fake:
        def __init__(self, *a, **k):
            log.opened.append(self)

        def close(self):
            pass

        def synchronize(self):
            pass

    class Context(Fake):
        def __init__(self, device=0, stream=None):
            super().__init__()
            self.device, self.handle = device, 1

    @recorded(log, "perform", "perform_raw", "perform_detect", "perform_fold", "set_kernel", "set_guppi")
    class Filterbank(Fake):
        nkeep, nsamp_step, nsamp_overlap, nsamp_fft = 100, 3200, 320, 3520

        def setup(self, *a, **k):
            return self

        def fold_is_fused(self):
            return 1

        def set_twobit(self, nsample, nlow_min, nlow_max, levels, table_type):
            log.call(self, "set_twobit", nsample, nlow_min, nlow_max, np.asarray(levels).shape, table_type)
            self.nsample, self.unpacked = nsample, 0

        def unpack_twobit(self, raw, first_sample, npart):
            """the rows and all-one weights of the windows the block touches; block ZERO_WEIGHT_BLOCK has one zero window"""
            log.call(self, "unpack_twobit", raw, first_sample, npart)
            nsamp = npart * self.nsamp_step + self.nsamp_overlap
            weights = torch.ones((2, -(-(first_sample + nsamp) // self.nsample)), dtype=torch.int32)
            if self.unpacked == ZERO_WEIGHT_BLOCK:
                weights[0, 3] = 0
            self.unpacked += 1
            return torch.zeros((1, 2, nsamp)), self.nsamp_step, weights

    class Conv(Filterbank):
        nkeep, nsamp_step, nsamp_overlap, nsamp_fft = 100, 100, 20, 120

    @recorded(log, "set_shape", "set_nbin", "set_ndat", "fold", "fold_moments", "fold_zeroed", "zero")
    class Fold(Fake):
        def set_bins(self, phi, phase_per_sample, ndat, idat_start=0, hits=None, **weights):
            log.call(self, "set_bins", phi, phase_per_sample, ndat, idat_start, hits, **weights)
            if hits is not None:
                hits[(ndat + idat_start) % len(hits)] += ndat             # (a count the books can be checked by)
            return ndat

        @staticmethod
        def fold_many(folds, inp):
            log.call("FoldEngine", "fold_many", folds, inp)

        def get_profiles_ptr(self):
            return 0

    class Cyclic(Fold):
        def set_shape(self, nchan, npol_in, npol_out, nlag, mover, nbin):
            log.call(self, "set_shape", nchan, npol_in, npol_out, nlag, mover, nbin)
            self.out = (nchan * (2 * nlag - 2) // mover, npol_out, nbin)

        def synch(self):
            log.call(self, "synch")
            return np.zeros(self.out, np.float32)

    @recorded(log, "zero")
    class Plfb(Fake):
        def set_shape(self, nchan_in, npol_in, ndim_in, nchan, npol_out, nbin):
            log.call(self, "set_shape", nchan_in, npol_in, ndim_in, nchan, npol_out, nbin)
            self.out = (nchan_in * nchan, npol_out, nbin)

        def accumulate(self, inp, ndat, idat_start, bins):
            log.call(self, "accumulate", inp, ndat, idat_start, bins)
            return len(bins)

        def synch(self):
            log.call(self, "synch")
            return np.zeros(self.out, np.float32)

    @recorded(log, "set_shape", "set_options", "transform")
    class Sk(Fake):
        def get_statistics(self):
            log.call(self, "get_statistics")
            return {"zapped": 0}

    class Delay(Fake):
        def __init__(self, ctx, delays, npol=1, absolute=False):
            super().__init__()
            d = np.asarray(delays, np.int64)
            self.zero_delay = 0 if absolute else int(d.max())
            self.total_delay = int(d.max()) if absolute else int((self.zero_delay - d).max())

        def transform(self, inp, out=None):
            log.call(self, "transform", inp)
            return max(0, inp.shape[2] - self.total_delay)

    @recorded(log, "polarimetry")
    class Detection(Fake):
        pass

    @recorded(log, "write")
    class Dump(Fake):
        def __init__(self, path, **k):
            super().__init__()

    for name, cls in (("Context", Context), ("FilterbankEngine", Filterbank), ("ConvolutionEngine", Conv), ("FoldEngine", Fold),
                      ("CyclicFoldEngine", Cyclic), ("PhaseLockedFilterbankEngine", Plfb), ("SpectralKurtosisEngine", Sk),
                      ("SampleDelay", Delay), ("DetectionEngine", Detection)):
        mp.setattr(pipeline, name, cls)
    mp.setattr(dada, "Dump", Dump)
    mp.setattr(pipeline, "_device_empty",
               lambda ctx, shape, dtype="float32", zero=False: torch.zeros(shape, dtype=getattr(torch, dtype)))
    mp.setattr(pipeline, "move_tail_fpt", lambda ctx, buf, dst, src, n, unit=1: log.call("pipeline", "move_tail_fpt", buf, dst, src, n, unit))
    mp.setattr(pipeline, "fourth_moment", lambda ctx, inp, out, ndat=None: log.call("pipeline", "fourth_moment", inp, out, ndat))
    mp.setattr(pipeline, "unpack_sigproc_fpt", lambda ctx, raw, rows, nbit, nchan, npol, ndat:
               log.call("pipeline", "unpack_sigproc_fpt", raw, rows, nbit, nchan, npol, ndat))

    def profiles_tensor(self, pulsar=None):
        nbin = self.cfg.nbin if pulsar is None else pulsar.nbin
        log.call("LoadToFold", "profiles_tensor", None if pulsar is None else self.pulsars.index(pulsar))
        return torch.zeros(self.nchan_out * nbin * (14 if self.moments else self.npol_out * self.cfg.ndim))
    mp.setattr(pipeline.LoadToFold, "profiles_tensor", profiles_tensor)
    return log


# 16 channels of a 32 MHz real band: 1 MHz, a block of 3 parts is 300 output samples, -L 450 us puts a boundary inside block 1,
# one at the end of block 2 and none in blocks 0 and 3
INFO = dict(centre_frequency=1382.0, bandwidth=-16.0, tsamp_us=1.0 / 32.0, machine="DADA")
CFG = dict(nchan=16, dispersion_measure=3.0, nbin=64, folding_period=0.004, ndim=4, parts_per_block=3, max_parts=2, subint_seconds=0.00045)
# -s: turns of 400 and of 230 samples -- in a block of 300, one pulsar has a single piece where the other has two
TARGETS = [pipeline.FoldTarget("a", folding_period=0.0004, nbin=64), pipeline.FoldTarget("b", folding_period=0.00023, nbin=32)]
# two complex channels of 16 MHz (the same 1 MHz output channels) as heaps and as GUPPI raw blocks; 16 detected channels of 1 MHz
HEAPS = dict(INFO, centre_frequency=1400.0, bandwidth=-32.0, nchan=2, ndim=2, tsamp_us=1.0 / 16.0, machine="MKBF")
GUPPI = dict(HEAPS, machine="GUPPI", guppi=(64, 288, 576))
DETECTED = dict(INFO, nchan=16, tsamp_us=1.0, machine="FAKE", detected="PPQQ")


def _fold(cfg=(), info=INFO, **kw):
    return lambda: pipeline.LoadToFold(pipeline.Config(**{**CFG, **dict(cfg)}), pipeline.InputInfo(**info), **kw)


MODES = {
    "during": _fold(),
    "during_K": _fold(dict(interchan_dedispersion=True)),
    "during_taps": _fold(dump_before=("Detection", "Fold")),
    "two_targets_s": _fold(dict(folding_period=0.0, subint_seconds=0.0, subint_turns=1.0), targets=TARGETS),
    "fourth_moment": _fold(dict(fourth_moment=True, ndim=2)),
    "after": _fold(dict(convolve_when="after")),
    "before": _fold(dict(convolve_when="before", freq_res=32768)),
    "cyclic": _fold(dict(nbin=32, cyclic_nchan=16, cyclic_mover=2, cyclic_npol=2)),
    "plfb": _fold(dict(nchan=8, folding_period=0.0004, plfb_nbin=8, plfb_nchan=64, subint_seconds=0.0)),
    "sk": _fold(dict(sk_zap=True)),
    # every input form through process_block: MeerKAT heaps (two channels of 16 MHz; 32 output channels), GUPPI raw blocks of 64 kept
    # samples per run (8 more overlap the next block), CPSR2's two-bit samples, and detected rows (a part is one spectrum)
    "heaps": _fold(dict(nchan=32), HEAPS),
    "heaps_subband": _fold(dict(nchan=32), HEAPS, subband=1),
    "guppi": _fold(dict(nchan=32), GUPPI),
    "guppi_subband": _fold(dict(nchan=32), GUPPI, subband=1),
    "twobit": _fold(info=dict(INFO, nbit=2, machine="CPSR2")),
    "detected": _fold(dict(parts_per_block=300, interchan_dedispersion=True), DETECTED),
    "detected_plain": _fold(dict(parts_per_block=300), DETECTED),
}
# where in its first heap / raw block / excision window each of the four blocks begins (every other mode: at 0), and the parts of the
# blocks of spectra
FIRST = {"heaps": (0, 128, 0, 255), "heaps_subband": (0, 128, 0, 255), "guppi": (0, 63, 17, 5), "guppi_subband": (0, 63, 17, 5),
         "twobit": (0, 384, 256, 128)}
SPECTRA = (300, 300, 300, 200)
ZERO_WEIGHT_BLOCK = 1                          # the two-bit block whose unpacker returns a zero weight (it also holds a boundary)


def _books(acc):
    hits = np.asarray(acc.hits)
    return {"hits_shape": list(hits.shape), "hits_sum": int(hits.sum(dtype=np.uint64)), "hits_nonzero": [int(i) for i in np.flatnonzero(hits)][:32],
            "integration_length": repr(float(acc.integration_length)), "ndat_total": int(acc.ndat_total),
            "subints": [{"keys": sorted(s), "hits_sum": int(np.asarray(s["hits"]).sum(dtype=np.uint64)), "ndat_total": int(s["ndat_total"]),
                         "integration_length": repr(float(s["integration_length"]))} for s in acc.subints]}


def _run(mp, mode):
    """Four blocks and a finish_subint of `mode`: the trace and the books, as the fixture holds them."""
    log = _fakes(mp)
    lt = MODES[mode]()
    opened = [log.name(o) for o in log.opened]
    marks = []
    for npart, first in zip(SPECTRA if mode.startswith("detected") else PARTS, FIRST.get(mode, (0, 0, 0, 0))):
        marks.append(len(log.calls))
        raw = torch.zeros(lt.block_bytes(npart, first) if first else lt.block_bytes(npart), dtype=torch.int8)
        lt.process_block(raw, npart, first_sample=first)
    marks.append(len(log.calls))
    lt.finish_subint()
    result = {"opened": opened, "blocks": [log.calls[a:b] for a, b in zip(marks, marks[1:])], "finish": log.calls[marks[-1]:],
              "books": _books(lt), "pulsars": [_books(p) for p in lt.pulsars], "ndat_out": int(lt.ndat_out), "nsamples_in": int(lt.nsamples_in)}
    forms = [c for c in log.calls[:marks[0]] if c[1] in ("set_guppi", "set_twobit")]
    if forms:                                  # what the constructor told the front end about the input's form
        result["form"] = forms
    if lt.twobit is not None:
        result["twobit"] ={k: int(getattr(lt.twobit, k)) for k in ("discarded_weights", "blocks_fused", "blocks_weighted")}
    lt.close()
    return json.loads(json.dumps(result))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_trace_of_four_blocks_is_the_recorded_one(monkeypatch, mode):
    with open(os.path.join(GOLDEN, mode + ".json")) as f:
        want = json.load(f)
    got = _run(monkeypatch, mode)
    assert got["opened"] == want["opened"]
    for k, (g, w) in enumerate(zip(got["blocks"], want["blocks"])):
        for i, (cg, cw) in enumerate(zip(g, w)):
            assert cg == cw, "block %d, call %d" % (k, i)
        assert len(g) == len(w), "block %d" % k
    assert got["finish"] == want["finish"]
    for key in ("books", "pulsars", "ndat_out", "nsamples_in"):
        assert got[key] == want[key], key
    assert got.get("twobit") == want.get("twobit") and got.get("form") == want.get("form")


def test_the_blocks_chosen_reach_the_branches():
    """what the fixtures are worth: a block with a boundary inside, one with a boundary at its end, one without; a fused and an
    unfused block; a pulsar folded with the others and one folded alone; a window and a part of M samples carried over a block"""
    def fixture(mode):
        with open(os.path.join(GOLDEN, mode + ".json")) as f:
            return json.load(f)
    methods = lambda block: [c[1] for c in block]
    during = fixture("during")
    assert [methods(b).count("perform_fold") for b in during["blocks"]] == [1, 0, 1, 1]
    assert [methods(b).count("profiles_tensor") for b in during["blocks"]] == [0, 1, 1, 0] and len(during["books"]["subints"]) == 3
    two = fixture("two_targets_s")
    assert any("fold_many" in methods(b) and "fold" in methods(b) for b in two["blocks"])
    assert all(len(p["subints"]) >= 2 for p in two["pulsars"])
    for mode in ("during_K", "plfb", "sk"):
        assert all("move_tail_fpt" in methods(b) for b in fixture(mode)["blocks"][:3]), mode
    assert fixture("sk")["ndat_out"] == (1100 // 128) * 128 and fixture("during_K")["ndat_out"] < 1100
    assert sum(methods(b).count("accumulate") for b in fixture("plfb")["blocks"]) >= 3
    # the input forms: a layout word per block, a sub-band rank's own geometry and shorter blocks, fused and weighted two-bit blocks
    layouts = lambda mode: [c[3]["layout"] for b in fixture(mode)["blocks"] for c in b if "layout" in c[3]]
    raw = lambda mode: [next(c[3]["raw"]["tensor"][0] for c in b if "raw" in c[3]) for b in fixture(mode)["blocks"]]
    for mode in ("heaps", "heaps_subband"):
        assert layouts(mode) == [3, 3 | 128 << 8, 3, 3 | 255 << 8], mode
    for mode in ("guppi", "guppi_subband"):
        assert layouts(mode) == [6, 6 | 63 << 8, 6 | 17 << 8, 6 | 5 << 8], mode
    assert fixture("guppi")["form"][0][2] == [64, 288, 576] and fixture("guppi_subband")["form"][0][2] == [64, 288, 288]
    assert all(a > b for mode in ("heaps", "guppi") for a, b in zip(raw(mode), raw(mode + "_subband")))
    two = fixture("twobit")
    assert two["twobit"]["blocks_fused"] >= 1 and two["twobit"]["blocks_weighted"] == 1 == two["twobit"]["discarded_weights"]
    assert any("weights" in c[3] for b in two["blocks"] for c in b if c[1] == "set_bins")
    assert all(methods(b)[0] == "unpack_sigproc_fpt" for mode in ("detected", "detected_plain") for b in fixture(mode)["blocks"])
    assert all("move_tail_fpt" in methods(b) for b in fixture("detected")["blocks"][:3])
    assert not any("move_tail_fpt" in methods(b) for b in fixture("detected_plain")["blocks"])


def regenerate():
    os.makedirs(GOLDEN, exist_ok=True)
    for mode in sorted(MODES):
        with pytest.MonkeyPatch.context() as mp:
            result = _run(mp, mode)
        with open(os.path.join(GOLDEN, mode + ".json"), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print("%s: %d calls" % (mode, sum(len(b) for b in result["blocks"]) + len(result["finish"])))


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_pipeline_trace_host.py --regenerate")
    regenerate()
