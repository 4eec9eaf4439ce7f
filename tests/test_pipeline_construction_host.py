"""Construction and release of the five pipeline drivers, on the host: every engine, the context and the device allocator of
dspsr_amd.pipeline are replaced by recording fakes, so what is opened, what is closed and in which order can be counted here."""
import itertools

import numpy as np
import pytest

from dspsr_amd import DspsrAmdError, pipeline

NKEEP, STEP, OVERLAP = 100, 3200, 320          # what the fake filterbank reports (block of 3 parts: 300 output samples)


class Log:
    def __init__(self):
        self.opened, self.closed, self.set_shapes = [], [], 0
        self.fail_set_shape = 0                  # the n-th FoldEngine.set_shape raises
        self.fail_rescale = False
        self.fail_sk_shape = False               # SpectralKurtosisEngine.set_shape raises
        self.fail_digitizer = False


def _fakes(monkeypatch, with_dump=False):
    log = Log()

    class Fake:
        def __init__(self, *a, **k):
            self.args = a
            log.opened.append(self)

        def close(self):
            log.closed.append(self)

        def synchronize(self):
            pass

    class Context(Fake):
        def __init__(self, device=0, stream=None):
            super().__init__()
            self.device, self.handle = device, 1

    class Filterbank(Fake):
        nkeep, nsamp_step, nsamp_overlap, nsamp_fft = NKEEP, STEP, OVERLAP, STEP + OVERLAP

        def setup(self, *a, **k):
            return self

        def fold_is_fused(self):
            return 1

    class Fold(Fake):
        def set_shape(self, *a):
            log.set_shapes += 1
            if log.set_shapes == log.fail_set_shape:
                raise DspsrAmdError("fake FoldEngine.set_shape refuses")

    class Sk(Fake):
        def set_shape(self, *a):
            if log.fail_sk_shape:
                raise DspsrAmdError("fake SpectralKurtosisEngine.set_shape refuses")

        def set_options(self, *a):
            pass

    class Delay(Fake):
        total_delay, zero_delay = 7, 11

    class Rescale(Fake):
        def __init__(self, *a, **k):
            if log.fail_rescale:
                raise DspsrAmdError("fake Rescale refuses")
            super().__init__(*a, **k)

    class Digitizer(Fake):
        def __init__(self, *a, **k):
            if log.fail_digitizer:
                raise DspsrAmdError("fake FITSDigitizer refuses")
            super().__init__(*a, **k)

    for name, cls in (("Context", Context), ("FilterbankEngine", Filterbank), ("ConvolutionEngine", type("Conv", (Filterbank,), {})),
                      ("FoldEngine", Fold), ("CyclicFoldEngine", type("Cyclic", (Fold,), {})),
                      ("PhaseLockedFilterbankEngine", type("Plfb", (Fold,), {})), ("SpectralKurtosisEngine", Sk), ("SampleDelay", Delay),
                      ("Rescale", Rescale), ("FITSDigitizer", Digitizer)):
        monkeypatch.setattr(pipeline, name, cls)
    monkeypatch.setattr(pipeline, "_device_empty", lambda ctx, shape, dtype="float32", zero=False: np.zeros(shape, dtype=dtype))
    if with_dump:
        from dspsr_amd import dada
        monkeypatch.setattr(dada, "Dump", type("Dump", (Fake,), {}))
    return log


def _released(log):
    """everything opened was closed exactly once, the context last"""
    assert log.opened and type(log.opened[0]).__name__ == "Context"
    assert sorted(map(id, log.closed)) == sorted(map(id, log.opened)) and len(set(map(id, log.closed))) == len(log.closed)
    assert log.closed[-1] is log.opened[0]
    return True


INFO = dict(centre_frequency=1382.0, bandwidth=-16.0, tsamp_us=1.0 / 32.0, machine="DADA")
CFG = dict(nchan=16, dispersion_measure=3.0, nbin=64, folding_period=0.004, ndim=4, parts_per_block=3, max_parts=2)
TWO = dict(INFO, centre_frequency=1400.0, bandwidth=-32.0, nchan=2, ndim=2, tsamp_us=1.0 / 16.0)
TARGETS = [pipeline.FoldTarget("a", folding_period=0.004, nbin=64), pipeline.FoldTarget("b", folding_period=0.00123, nbin=32)]
SEARCH_INFO = dict(centre_frequency=1382.0, bandwidth=-400.0, nchan=1, npol=2, ndim=1, tsamp_us=0.00125, machine="DADA")
COHERENT = dict(nchan=64, tscrunch=16, nbit=8, rescale_seconds=2e-4, freq_res=1024, parts_per_block=3, max_parts=4)
DIRECT_INFO = dict(centre_frequency=1400.0, bandwidth=-8.0, nchan=8, npol=2, ndim=2, tsamp_us=1.0, machine="DADA")
# digifits on the same inputs: -F 64:D -K at 16 filterbank samples per output sample, and no -F
FITS_F_K = dict(nchan=64, convolve=True, dispersion_measure=0.03, coherent_dedisp=True, dedisperse=True, tsamp=2.56e-6, npol=2, nbit=8, nsblk=16,
                parts_per_block=3, max_parts=4)
FITS_DIRECT = dict(nchan=0, tsamp=4e-6, npol=2, nbit=8, nsblk=16, parts_per_block=2048)
DIRECT = dict(tscrunch=4, nbit=8, rescale_seconds=256.5 * 4 / 1e6, parts_per_block=2048, dispersion_measure=20.0, dedisperse=True)


def _fold(cfg=(), info=INFO, **kw):
    return lambda: pipeline.LoadToFold(pipeline.Config(**{**CFG, **dict(cfg)}), pipeline.InputInfo(**info), **kw)


BUILDS = {
    "during": (_fold(), "Context Filterbank Fold"),
    "during_K": (_fold(dict(interchan_dedispersion=True)), "Context Filterbank Fold Delay"),
    "during_subband": (_fold(dict(nchan=32), TWO, subband=1), "Context Filterbank Fold"),
    "during_subband_K": (_fold(dict(nchan=32, interchan_dedispersion=True, freq_res=256), TWO, subband=1), "Context Filterbank Fold Delay"),
    "during_taps": (_fold(dump_before=("Detection", "Fold")), "Context Filterbank Fold Dump Dump"),
    "after": (_fold(dict(convolve_when="after")), "Context Filterbank Conv Fold"),
    "never": (_fold(dict(convolve_when="never")), "Context Filterbank Fold"),
    "before": (_fold(dict(convolve_when="before", freq_res=32768)), "Context Conv Filterbank Fold"),
    "cyclic": (_fold(dict(nbin=32, cyclic_nchan=16, cyclic_mover=2, cyclic_npol=2)), "Context Filterbank Cyclic"),
    "plfb": (_fold(dict(nchan=8, folding_period=0.0004, plfb_nbin=8, plfb_nchan=64)), "Context Filterbank Plfb"),
    "sk": (_fold(dict(sk_zap=True)), "Context Filterbank Fold Sk"),
    "two_targets": (_fold(dict(folding_period=0.0), targets=TARGETS), "Context Filterbank Fold Fold Fold"),
    "fourth_moment": (_fold(dict(fourth_moment=True, ndim=2)), "Context Filterbank Fold"),
    "LoadToFil": (lambda: pipeline.LoadToFil(pipeline.SearchConfig(nchan=64, tscrunch=16, nbit=8, rescale_seconds=2e-4, parts_per_block=32),
                                             pipeline.InputInfo(**SEARCH_INFO)), "Context Rescale"),
    "LoadToFilCoherent": (lambda: pipeline.LoadToFilCoherent(pipeline.SearchConfig(dispersion_measure=0.03, dedisperse=True, fscrunch=4, **COHERENT),
                                                             pipeline.InputInfo(**SEARCH_INFO)), "Context Filterbank Delay Rescale"),
    "LoadToFilDirect": (lambda: pipeline.LoadToFilDirect(pipeline.SearchConfig(**DIRECT), pipeline.InputInfo(**DIRECT_INFO)),
                        "Context Delay Rescale"),
    "LoadToFITS_F_K": (lambda: pipeline.LoadToFITS(pipeline.FitsConfig(**FITS_F_K), pipeline.InputInfo(**SEARCH_INFO)),
                       "Context Filterbank Delay Digitizer"),
    "LoadToFITS_direct": (lambda: pipeline.LoadToFITS(pipeline.FitsConfig(**FITS_DIRECT), pipeline.InputInfo(**DIRECT_INFO)), "Context Digitizer"),
}


@pytest.mark.parametrize("name", sorted(BUILDS))
def test_construction_completes_and_close_releases_everything_once(monkeypatch, name):
    log = _fakes(monkeypatch, with_dump=True)
    build, opened = BUILDS[name]
    drv = build()
    assert " ".join(type(o).__name__ for o in log.opened) == opened
    if name == "two_targets":                            # the single-pulsar fold went when the pulsars got theirs
        assert len(drv.pulsars) == 2 and drv.fold is None and log.closed == [log.opened[2]]
    if name == "during_subband_K":                       # the band's head room; this rank's SampleDelay (total_delay 7) gives up the rest
        assert drv.sd_short == drv.sd_head - 7 > 0
    if name not in ("LoadToFil", "LoadToFilDirect", "LoadToFITS_F_K", "LoadToFITS_direct", "after", "never", "before"):      # (the two wrappers scale the engine's numbers)
        assert (drv.nkeep, drv.nsamp_step, drv.nsamp_overlap) == (NKEEP, STEP, OVERLAP)
    drv.close()
    assert _released(log)
    n = len(log.closed)
    drv.close()
    assert len(log.closed) == n


def test_load_to_fold_defaults_are_set_on_every_path(monkeypatch):
    """the fields the class reads later exist whatever the path (sd_short was missing from three of five constructors)"""
    _fakes(monkeypatch)
    for name in ("during", "during_K", "after", "never", "before", "cyclic", "plfb", "sk", "two_targets", "fourth_moment"):
        lt = BUILDS[name][0]()
        assert (lt.sd_carried, lt.sd_short, lt.fused_fold, lt.integration_length, lt.ndat_total, lt.nsamples_in, lt.ndat_out) == \
            (0, 0, lt.fused_mode != 0, 0.0, 0, 0, 0)
        assert lt.optime == {} and lt.subints == [] and lt.dumps == {} and lt._turns is None and lt._moment_rows is None
        assert lt.sd_head == (0 if name != "during_K" else lt.sd.head) and lt.hits.dtype == np.uint32 and not lt.hits.any()
        lt.close()


FAILURES = {
    "LoadToFold_K_exceeds": (_fold(dict(interchan_dedispersion=True, dispersion_measure=30.0)), {},
                             "dspsr_amd.LoadToFold: inter-channel delay of 1415 samples exceeds the block of 300"),
    "LoadToFilCoherent_K_exceeds": (lambda: pipeline.LoadToFilCoherent(pipeline.SearchConfig(dispersion_measure=0.25, dedisperse=True, **COHERENT),
                                                                       pipeline.InputInfo(**SEARCH_INFO)), {},
                                    "dspsr_amd.LoadToFilCoherent: inter-channel delay of 2016 samples exceeds the block of 300"),
    "second_target_set_shape": (BUILDS["two_targets"][0], dict(fail_set_shape=3), "fake FoldEngine.set_shape refuses"),
    "sk_set_shape": (BUILDS["sk"][0], dict(fail_sk_shape=True), "fake SpectralKurtosisEngine.set_shape refuses"),
    "LoadToFil_rescale": (BUILDS["LoadToFil"][0], dict(fail_rescale=True), "fake Rescale refuses"),
    "LoadToFilCoherent_rescale": (BUILDS["LoadToFilCoherent"][0], dict(fail_rescale=True), "fake Rescale refuses"),
    "LoadToFilDirect_rescale": (BUILDS["LoadToFilDirect"][0], dict(fail_rescale=True), "fake Rescale refuses"),
    "LoadToFITS_digitizer": (BUILDS["LoadToFITS_F_K"][0], dict(fail_digitizer=True), "fake FITSDigitizer refuses"),
}


@pytest.mark.parametrize("name", sorted(FAILURES))
def test_a_failure_during_construction_releases_what_was_opened(monkeypatch, name):
    log = _fakes(monkeypatch)
    build, faults, message = FAILURES[name]
    for k, v in faults.items():
        setattr(log, k, v)
    with pytest.raises(DspsrAmdError, match=message):
        build()
    assert _released(log)
    if name == "second_target_set_shape":                # context, filterbank, the first fold, both pulsars' folds
        assert [type(o).__name__ for o in log.opened] == ["Context", "Filterbank", "Fold", "Fold", "Fold"]
    if name == "sk_set_shape":                           # the engine that refused was opened, and is released with the rest
        assert [type(o).__name__ for o in log.opened] == ["Context", "Filterbank", "Fold", "Sk"]


REFUSALS = [
    (_fold(info=dict(INFO, npol=1)), "dsp::Detection::polarimetry Cannot detect polarization when npol != 2"),
    (_fold(dict(convolve_when="sometimes")), "convolve_when='sometimes' is not one of during / after / before / never"),
    (_fold(info=dict(INFO, nchan=3)), "output nchan=16 not a multiple of input nchan=3"),
    (_fold(dict(nchan=32), TWO, subband=2), "subband=2 outside the 2 input channels"),
    (_fold(dict(nchan=32, convolve_when="after"), TWO, subband=0), r"sub-band sharded runs are built for -F N:D \(convolve_when = during\)"),
    (_fold(dict(convolve_when="after", interchan_dedispersion=True)), r"-K and the dump taps are built for -F N:D \(convolve_when = during\)"),
    (_fold(dict(convolve_when="before"), dump_before=("Fold",)), r"-K and the dump taps are built for -F N:D \(convolve_when = during\)"),
    (_fold(dump_before=("Fold", "Unpacker")), r"insert_dump_point no operation named 'Unpacker' on this path \(Detection, Fold\)"),
    (_fold(dict(interchan_dedispersion=True), dump_before=("Fold", "Detection")), "the pre_Detection tap is not built for -K"),
    (_fold(dict(folding_period=0.0)), "dsp::Fold::fold no polynomial and no period specified"),
    (lambda: pipeline.LoadToFilCoherent(pipeline.SearchConfig(dispersion_measure=2.0, fscrunch=5, **COHERENT), pipeline.InputInfo(**SEARCH_INFO)),
     "dspsr_amd.LoadToFilCoherent: nchan=64 is not a multiple of fscrunch=5"),
    (lambda: pipeline.LoadToFilCoherent(pipeline.SearchConfig(dispersion_measure=2.0, **{**COHERENT, "rescale_seconds": 1e-9}),
                                        pipeline.InputInfo(**SEARCH_INFO)), "dsp::Rescale::init nsample == 0"),
    (lambda: pipeline.LoadToFil(pipeline.SearchConfig(nchan=64, tscrunch=16, rescale_seconds=1e-9, parts_per_block=32),
                                pipeline.InputInfo(**SEARCH_INFO)), "dsp::Rescale::init nsample == 0"),
    # LoadToFITS: a refusal of its front end, and one of its own
    (lambda: pipeline.LoadToFITS(pipeline.FitsConfig(**FITS_DIRECT), pipeline.InputInfo(**dict(DIRECT_INFO, machine="CASPSR"))),
     "dspsr_amd.LoadToFilDirect: the CASPSR byte order is not built on this path"),
    (lambda: pipeline.LoadToFITS(pipeline.FitsConfig(**dict(FITS_F_K, nbit=3)), pipeline.InputInfo(**SEARCH_INFO)),
     "dsp::FITSDigitizer::set_nbit nbit=3 not understood"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_come_before_any_device(monkeypatch, case):
    log = _fakes(monkeypatch, with_dump=True)
    build, message = REFUSALS[case]
    with pytest.raises(DspsrAmdError, match=message):
        build()
    assert log.opened == []                              # not even the context


def test_a_refusal_that_won_before_still_wins(monkeypatch):
    """two refusals on one input: the earlier of the old constructor's order is the one raised"""
    _fakes(monkeypatch)
    with pytest.raises(DspsrAmdError, match="subband=5 outside"):                 # ... and npol != 2
        _fold(dict(nchan=32), dict(TWO, npol=1), subband=5)()
    with pytest.raises(DspsrAmdError, match="npol != 2"):                         # ... and a bad convolve_when, and nchan % input nchan
        _fold(dict(convolve_when="x"), dict(INFO, npol=1, nchan=3))()
    with pytest.raises(DspsrAmdError, match="not one of during"):                 # ... and nchan % input nchan
        _fold(dict(convolve_when="x"), dict(INFO, nchan=3))()
    with pytest.raises(DspsrAmdError, match="not a multiple of input nchan"):     # ... and -K with `after`
        _fold(dict(convolve_when="after", interchan_dedispersion=True), dict(INFO, nchan=3))()
    with pytest.raises(DspsrAmdError, match="sub-band sharded runs are built"):   # ... and -K with `after`
        _fold(dict(nchan=32, convolve_when="after", interchan_dedispersion=True), TWO, subband=0)()


def test_close_on_an_instance_that_never_opened_a_device():
    """close() after a refusal of the host plan, and the communicator setters on a bare instance (test_fold_many_host uses them so)"""
    for cls in (pipeline.LoadToFil, pipeline.LoadToFilCoherent, pipeline.LoadToFilDirect, pipeline.LoadToFITS):
        drv = cls.__new__(cls)
        drv.close()
        drv.close()
    lt = pipeline.LoadToFold.__new__(pipeline.LoadToFold)
    lt.pulsars = [object(), object()]
    with pytest.raises(DspsrAmdError, match="one pulsar"):
        lt.set_communicator(None, 0, 2)
    lt._defaults()
    lt.close()
    lt.close()


# ---- the -K carry ------------------------------------------------------------------------------------------------------

def _site(head, carried, nd, guarded):
    """The arithmetic the three -K call sites had, restated: the -K chain of LoadToFold and LoadToFilCoherent.detect_scrunch
    (guarded False), LoadToFilDirect.detect_scrunch (guarded True: no transform without samples, no move onto itself).
    Returns (off, nin, nout, move or None, carried)."""
    off, nin = head - carried, carried + nd
    nout = max(0, nin - head) if (nin or not guarded) else 0
    carry = nin - nout
    move = (head - carry, off + nout, carry) if carry and not (guarded and off + nout == head - carry) else None
    return off, nin, nout, move, carry


@pytest.mark.parametrize("ndim", [1, 4])
@pytest.mark.parametrize("head,short", [(0, 0), (1, 0), (5, 0), (1, 1), (5, 2)])       # (short: a sub-band rank of LoadToFold)
def test_delay_carry_against_the_three_call_sites(monkeypatch, head, short, ndim):
    moves = []
    monkeypatch.setattr(pipeline, "move_tail_fpt", lambda ctx, buf, dst, src, n, unit=1: moves.append((dst, src, n, unit)))
    lengths = sorted({0, 1, head, head + 3})
    for blocks in itertools.product(lengths, repeat=3):
        sd = pipeline.DelayCarry()
        sd.head, sd.short = head, short
        buf = np.arange(2 * 3 * (2 * head + 3) * ndim, dtype=np.float32).reshape(2, 3, -1)
        carried = 0
        for nd in blocks:
            off, nin, nout, move, carry = _site(head, carried, nd, guarded=True)
            if nd:                                       # (the two unguarded callers never pass an empty block)
                assert (off, nin, nout, move, carry) == _site(head, carried, nd, guarded=False)
            rows = sd.rows(buf, nd, ndim)
            nuse = max(0, nin - short)
            assert rows.shape == (2, 3, nuse * ndim) and (nuse == 0 or rows[0, 0, 0] == off * ndim)
            got = max(0, nuse - (head - short)) if nuse else 0           # the transform of a SampleDelay whose total is head - short
            assert got == nout
            del moves[:]
            sd.keep_tail(None, buf, nd, got, ndim)
            assert moves == ([move + (ndim,)] if move else []) and sd.carried == carry
            assert all(dst != src and n > 0 for dst, src, n, _ in moves)
            carried = carry


def _site_plfb(head, tail, ndat, keep):
    """The fourth site, as -G wrote it out by hand before it held a DelayCarry (complex rows: width 2): the new samples go to
    buf[:, :, 2 * head:], the rows begin at 2 * (head - tail), and the `keep` samples from the next window's start on move to the end
    of the head room.  Returns (new offset, rows offset, consumed, move or None, tail)."""
    move = (head - keep, head + ndat - keep, keep) if keep else None
    return 2 * head, 2 * (head - tail), tail + ndat - keep, move, keep


def _site_sk(head, tail, ndat, nuse):
    """The fifth site, as -skz wrote it out by hand: as -G, with `nuse` samples consumed (whole parts of M)."""
    keep = tail + ndat - nuse
    move = (head - keep, head - tail + nuse, keep) if keep else None
    return 2 * head, 2 * (head - tail), nuse, move, keep


@pytest.mark.parametrize("head", [1, 31, 64])
def test_delay_carry_against_the_plfb_and_sk_call_sites(monkeypatch, head):
    """-G and -skz hold the class that -K holds: with the three sites above, five.  Three blocks in a row, each consuming nothing
    (where the head room can hold all of it), a part, or all of what it has; what stays never exceeds the head room, as a window
    shorter than ndat_fft = head (-G) and a part shorter than M = head + 1 (-skz) never do.  Both sites always bring samples
    (ndat >= 1), so the class's guard against a move onto itself never fires: the moves are the same, one for one."""
    moves = []
    monkeypatch.setattr(pipeline, "move_tail_fpt", lambda ctx, buf, dst, src, n, unit=1: moves.append((dst, src, n, unit)))
    buf = np.arange(2 * 3 * (2 * head + 3) * 2, dtype=np.float32).reshape(2, 3, -1)
    seen = set()

    def walk(tail, blocks):
        if not blocks:
            return
        ndat, nin = blocks[0], tail + blocks[0]
        least = max(0, nin - head)                       # consumed: as little as the head room allows, a part, all
        for nout in sorted({least, (least + nin) // 2, nin}):
            seen.add("nothing" if not nout else "all" if nout == nin else "part")
            want = _site_sk(head, tail, ndat, nout)
            assert want == _site_plfb(head, tail, ndat, nin - nout)
            c = pipeline.DelayCarry(head=head)
            c.carried = tail
            new, rows = c.new(buf, 2), c.rows(buf, ndim=2)
            assert (new.shape[2], rows.shape[2]) == (buf.shape[2] - want[0], buf.shape[2] - want[1])
            assert new[0, 0, 0] == want[0] and rows[0, 0, 0] == want[1]
            assert c.rows(buf, ndat, 2).shape[2] == 2 * nin and c.rows(buf, ndat, 2)[0, 0, 0] == want[1]
            del moves[:]
            c.keep_tail(None, buf, ndat, nout, 2)
            assert moves == ([want[3] + (2,)] if want[3] else []) and c.carried == want[4] <= head
            walk(c.carried, blocks[1:])

    for blocks in itertools.product(sorted({1, head, head + 3}), repeat=3):
        walk(0, blocks)
    assert seen == {"nothing", "part", "all"}


def test_delay_carry_plans_zero_and_head_like_sample_delay():
    """SampleDelay::build (SampleDelay.C:75-99): zero_delay = the largest delay, total_delay = the largest applied one"""
    sd = pipeline.DelayCarry(np.array([3, -2, 7, 0]))
    assert (sd.zero, sd.head, sd.carried, sd.short) == (7, 9, 0, 0)
    sd.check_block("LoadToFold", 9)
    with pytest.raises(DspsrAmdError, match="dspsr_amd.LoadToFold: inter-channel delay of 9 samples exceeds the block of 8"):
        sd.check_block("LoadToFold", 8)
    assert (pipeline.DelayCarry().zero, pipeline.DelayCarry().head) == (0, 0)
