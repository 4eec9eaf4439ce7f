"""The pre-split spectrum of real dual-polarisation input (csrc/fb_row_map.h): pass 1 leaves the rows of A in mirror-paired
blocks, pass 2 forms the Hermitian split and stores the two polarisations, the inverse pass loads them ready.

Every case runs the same block twice -- with the object's default path, which must be the pre-split one, and with
split_in_inverse = 1, the path every other input keeps -- and requires the complex filterbank output of the two to be equal bit
for bit (the split evaluates the same expressions in the same order in either pass) and within the oracle bounds of
test_gpu_parity._fb_case.  The float64 reference of a case is computed once and shared by its two runs.

Geometries (C, M, nfilt), the smallest that reach each branch of the row map; T2 = min(M, 2^14 / (2 C)) rows per pass-2 tile:
  (1024, 16, (1, 2))         T2 = 8, two blocks: block 0 with rows 0 and M / 2, and the last block
  (1024, 64, (5, 6))         T2 = 8, eight blocks: regular middle blocks
  (2048, 16, (1, 2))         T2 = 4
  (4096, 16, (1, 2))         T2 = 2: block 0 is {0, M / 2}, every other block one mirror pair
  (16, 256, (20, 21))        T2 = M: the whole row set in one block; T3 = 16 channels per inverse tile; the kernels that take their
                             tile shape from the geometry
  (4, 4096, (422, 422))      T2 = M / 2, two blocks of 2048 rows; T3 = 2; the inverse pass of the headline
  (1024, 4096, (843, 844))   the full-tile instantiations the benchmark runs (T2 = 8, T3 = 2), two parts
M = 16 and M = 256 have a last pass-1 stage that does not step whole tile heights (the image index of every row from the map);
M = 64, 4096 take the two affine runs below and above row M / 2."""
import contextlib

import numpy as np
import pytest

from test_gpu_parity import _fb_block, _fb_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


@contextlib.contextmanager
def engines(split_in_inverse):
    """Every FilterbankEngine set up inside -- directly or by a pipeline -- gets `split_in_inverse`; yields the list of their
    presplit() answers."""
    from dspsr_amd import engine
    orig = engine.FilterbankEngine.setup
    taken = []

    def setup(self, *a, **kw):
        kw["split_in_inverse"] = split_in_inverse
        r = orig(self, *a, **kw)
        taken.append(self.presplit())
        return r
    engine.FilterbankEngine.setup = setup
    try:
        yield taken
    finally:
        engine.FilterbankEngine.setup = orig


class OracleOnce:
    """The oracle module with the float64 filterbank output of a case computed by its first run and handed to the second (the
    two runs of a case differ in the object's path only)."""

    def __init__(self, o):
        self._o, self._ref = o, None

    def __getattr__(self, name):
        return getattr(self._o, name)

    def filterbank(self, *a, **kw):
        if self._ref is None:
            self._ref = self._o.filterbank(*a, **kw)
        return self._ref


class NoReference(OracleOnce):
    """... without the float64 filterbank: for the tests that compare two device outputs only"""

    def filterbank(self, *a, **kw):
        return None


def both_paths(oracle, gpu, C, M, nfilt, npart, presplit=True, **kw):
    """_fb_case (which asserts the oracle's bounds) on the default path and with the split forced into the inverse pass"""
    o = OracleOnce(oracle)
    with engines(False) as taken:
        new, _ = _fb_case(o, gpu, C, M, nfilt, npart, **kw)
    assert taken == [presplit], "path of the default object"
    with engines(True) as taken:
        old, _ = _fb_case(o, gpu, C, M, nfilt, npart, **kw)
    assert taken == [False], "split_in_inverse = 1 must keep the split in the inverse pass"
    assert np.array_equal(new, old)
    return new


GEOMETRIES = [
    (1024, 16, (1, 2), 2, 1),
    (1024, 64, (5, 6), 2, 1),
    (2048, 16, (1, 2), 2, 1),
    (4096, 16, (1, 2), 2, 1),
    (16, 256, (20, 21), 2, 1),
    (4, 4096, (422, 422), 2, 1),
    (1024, 4096, (843, 844), 2, 2),
]


@pytest.mark.parametrize("C,M,nfilt,npart,max_parts", GEOMETRIES)
def test_presplit_equals_the_split_in_the_inverse_pass(oracle, gpu, C, M, nfilt, npart, max_parts):
    both_paths(oracle, gpu, C, M, nfilt, npart, max_parts=max_parts)


@pytest.mark.parametrize("C,M,nfilt", [(1024, 16, (1, 2)), (16, 256, (20, 21))])
def test_a_group_of_four_parts_then_a_group_of_one(oracle, gpu, C, M, nfilt):
    both_paths(oracle, gpu, C, M, nfilt, 5, max_parts=4)


@pytest.mark.parametrize("C,M,nfilt", [(1024, 64, (5, 6)), (4, 4096, (422, 422))])
def test_caspsr_byte_order(oracle, gpu, C, M, nfilt):
    assert ((M - sum(nfilt)) * 2 * C) % 4 == 0          # (CASPSR blocks are regrouped only at part steps that are multiples of 4)
    both_paths(oracle, gpu, C, M, nfilt, 3, layout="caspsr", max_parts=2)


@pytest.mark.parametrize("C,M,nfilt", [(2048, 16, (1, 2)), (16, 256, (20, 21))])
def test_float32_rows(oracle, gpu, C, M, nfilt):
    # pass 1's generic loads (the other instantiation family of the row-mapped kernel)
    both_paths(oracle, gpu, C, M, nfilt, 2, use_raw=False, max_parts=2)


def test_complex_input_keeps_the_split_free_path(oracle, gpu):
    # complex dual-pol input: one sequence per polarisation, nothing to split; three passes (C = 32, M = 128)
    both_paths(oracle, gpu, 32, 128, (9, 10), 3, presplit=False, real=False, max_parts=2)


def test_odd_nchan_keeps_the_split_in_the_inverse_pass(oracle, gpu):
    # nchan_subband = 3 * 32: the sub-spectra pass through k_sub_combine in the X layout
    both_paths(oracle, gpu, 96, 256, (20, 21), 3, presplit=False, max_parts=2)


@pytest.mark.parametrize("ndim", [4, 2])
@pytest.mark.parametrize("C,M,nfilt", [(1024, 16, (1, 2)), (16, 256, (20, 21))])
def test_detected_output(oracle, gpu, C, M, nfilt, ndim):
    dspsr_amd, _ = gpu
    npart = 3
    got = []
    for old in (False, True):
        with engines(old) as taken:
            b = _fb_block(NoReference(oracle), gpu, C, M, nfilt, npart, max_parts=2)
        assert taken == [not old]
        det = torch.zeros((b.nchan, 4 // ndim, npart * b.plan.nkeep * ndim), dtype=torch.float32, device="cuda")
        b.eng.perform_detect(det, npart, dspsr_amd.COHERENCE, ndim, raw=b.raw, layout=b.layout, scale=b.scale)
        b.eng.finish()
        got.append(det.cpu().numpy())
        b.eng.close()
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0
    assert np.array_equal(got[0], got[1])


def test_load_to_fold_exact_fused_fold(gpu):
    """LoadToFold on a tiny geometry with the exact fused fold (FUSED_ALWAYS: mode 1, time-order sums), 5 parts per block in
    groups of four and one: profile and hits are bit-identical between the two paths."""
    from dspsr_amd import pipeline, synth
    freq, bw, tsamp, dm, period, nchan, nbin = 1382.0, -16.0, 1.0 / 32.0, 30.0, 0.004, 16, 64
    info = pipeline.InputInfo(centre_frequency=freq, bandwidth=bw, tsamp_us=tsamp, machine="DADA")
    dumps = []
    for old in (False, True):
        cfg = pipeline.Config(nchan=nchan, dispersion_measure=dm, nbin=nbin, folding_period=period, ndim=4,
                              parts_per_block=5, max_parts=4, fused_fold=True, force_fused=True)
        with engines(old) as taken:
            lt = pipeline.LoadToFold(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
        assert taken == [not old] and lt.fused_mode == 1
        nblocks = 2
        step = cfg.parts_per_block * lt.nsamp_step
        raw = synth.voltages(nblocks * step + lt.nsamp_overlap, freq, bw, tsamp, dm, period)
        d_raw = torch.from_numpy(raw).cuda()
        for blk in range(nblocks):
            lt.process_block(d_raw[2 * blk * step: 2 * (blk * step + step + lt.nsamp_overlap)])
        lt.finish_subint()
        lt.synchronize()
        dumps.append([(s["hits"].copy(), s["profile_dev"].cpu().numpy()) for s in lt.subints])
        lt.close()
    assert len(dumps[0]) == len(dumps[1]) >= 1
    for (h0, p0), (h1, p1) in zip(*dumps):
        assert h0.sum() > 0 and np.abs(p0).max() > 0
        assert np.array_equal(h0, h1) and np.array_equal(p0, p1)


def test_load_to_fil_search_epilogue(gpu):
    """LoadToFilCoherent (`digifil -F 64:D -x 1024 -t 16`) with detection and the time scrunch inside the inverse pass, two blocks of
    6 parts in groups of four and two: the packed bytes are equal between the two paths."""
    from dspsr_amd import pipeline
    rng = np.random.default_rng(46)
    info = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=-400.0, nchan=1, npol=2, ndim=1, tsamp_us=0.00125, machine="DADA")
    outs = []
    stream = None
    for old in (False, True):
        cfg = pipeline.SearchConfig(nchan=64, tscrunch=16, nbit=8, rescale_seconds=2e-4, dispersion_measure=2.0, freq_res=1024,
                                    parts_per_block=6, max_parts=4, npol=1)
        with engines(old) as taken:
            lf = pipeline.LoadToFilCoherent(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
        assert taken == [not old] and lf.fused
        nblk = 6 * lf.nsamp_step + lf.nsamp_overlap
        if stream is None:
            stream = np.clip(np.rint(rng.standard_normal((2 * 6 * lf.nsamp_step + lf.nsamp_overlap) * 2) * 24.0), -128, 127).astype(np.int8)
        got = []
        for blk in range(2):
            raw = stream[blk * 6 * lf.nsamp_step * 2:(blk * 6 * lf.nsamp_step + nblk) * 2]
            got.append(lf.process_block(torch.from_numpy(raw.copy()).cuda()).cpu().numpy().copy())
        lf.close()
        outs.append(got)
    for a, b in zip(*outs):
        assert a.size > 0 and np.array_equal(a, b)
