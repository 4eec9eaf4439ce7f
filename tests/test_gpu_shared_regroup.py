"""The shared row grid of the 8-bit regroup (csrc/fb_rt_layout.h, k_raw_transpose).

Parts of a launch group that start whole rows apart read their windows from ONE regrouped row grid; a group of one part, and a
group whose padded grid would be larger than its windows, keep one window per part.  Every case runs 5 parts with max_parts = 4
-- a shared group of four, then a group of one (per part) -- and must equal the same block run with max_parts = 1 (per part
throughout) bit for bit, and the float64 oracle at the bounds of test_gpu_parity._fb_case.  Input: real dual-pol 8-bit blocks in
the generic and in the CASPSR order (the two 8-bit loaders of k_raw_transpose).

The geometries are the smallest that reach each store branch of k_raw_transpose and each loader branch (tile columns T1 =
min(2 C, 2^14 / M)):
  (4, 4096, (422, 422))   T1 = 4: the 16-byte two-row store; nkeep even
  (4, 4096, (421, 422))   the same with nkeep odd: odd row shifts, an odd row count (the last block takes the 4-byte stores)
  (16, 256, (20, 21))     T1 = 32: 16 bytes of a row piece per lane; nkeep odd
  (4, 8192, (100, 101))   T1 = 2: 4-byte stores
  (2, 2048, (100, 50))    Rr = 4 < 8: the narrow loader
  (4, 16, (1, 2))         more workgroups than items in every pass; windows of 16 rows in a grid padded to 64

The per-part form inside a group of several parts: with raw input the part step is always nkeep * Rr, a whole number of rows
(dspsr_amd_filterbank_perform_raw takes no step; a caller-given step exists for float32 rows only, which k_float_transpose
regroups and this change leaves alone), so a step off the row grid cannot reach k_raw_transpose through the C-ABI -- that
refusal is checked on the host (tests/test_rt_layout_host.py).  What can be reached is the other refusal of rt_takes_shared:
two windows of 16 rows, whose grid of 29 rows padded to 64 would be larger than the two windows."""
import numpy as np
import pytest

from test_gpu_parity import _fb_case

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


GEOMETRIES = [
    (4, 4096, (422, 422)),
    (4, 4096, (421, 422)),
    (16, 256, (20, 21)),
    (4, 8192, (100, 101)),
    (2, 2048, (100, 50)),
    (4, 16, (1, 2)),
]


@pytest.mark.parametrize("layout", ["generic", "caspsr"])
@pytest.mark.parametrize("C,M,nfilt", GEOMETRIES)
def test_shared_group_equals_per_part_and_the_oracle(oracle, gpu, C, M, nfilt, layout):
    assert ((M - sum(nfilt)) * 2 * C) % 4 == 0          # (CASPSR blocks are regrouped only at part steps that are multiples of 4)
    shared, _ = _fb_case(oracle, gpu, C, M, nfilt, 5, layout=layout, max_parts=4)       # (asserts the oracle's bounds)
    single, _ = _fb_case(oracle, gpu, C, M, nfilt, 5, layout=layout, max_parts=1)
    assert np.array_equal(shared, single)


def test_complex_input_shares_one_grid_per_polarisation(oracle, gpu):
    # complex dual-pol 8-bit input on a 16-byte base (fb_pass1 fastc): one sequence per polarisation, each with its own row grid
    # (seq_stride); C = 32, M = 128: three passes, part step 109 * 32 samples = 109 rows
    a, _ = _fb_case(oracle, gpu, 32, 128, (9, 10), 5, real=False, max_parts=4)
    b, _ = _fb_case(oracle, gpu, 32, 128, (9, 10), 5, real=False, max_parts=1)
    assert np.array_equal(a, b)


def test_windows_shorter_than_their_padding_stay_per_part(oracle, gpu):
    a, _ = _fb_case(oracle, gpu, 4, 16, (1, 2), 2, max_parts=2)
    b, _ = _fb_case(oracle, gpu, 4, 16, (1, 2), 2, max_parts=1)
    assert np.array_equal(a, b)


def test_load_to_fold_exact_fused_fold_over_shared_groups(gpu):
    """LoadToFold on a tiny geometry with the exact fused fold (FUSED_ALWAYS: mode 1, time-order sums), 5 parts per block:
    profile and hits are bit-identical between max_parts 4 (a shared group of four and a group of one per block) and 1."""
    dspsr_amd, _ = gpu
    from dspsr_amd import pipeline, synth
    freq, bw, tsamp, dm, period, nchan, nbin = 1382.0, -16.0, 1.0 / 32.0, 30.0, 0.004, 16, 64
    info = pipeline.InputInfo(centre_frequency=freq, bandwidth=bw, tsamp_us=tsamp, machine="DADA")
    dumps = []
    for max_parts in (4, 1):
        cfg = pipeline.Config(nchan=nchan, dispersion_measure=dm, nbin=nbin, folding_period=period, ndim=4,
                              parts_per_block=5, max_parts=max_parts, fused_fold=True, force_fused=True)
        lt = pipeline.LoadToFold(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
        assert lt.fused_mode == 1
        nblocks = 2
        step = cfg.parts_per_block * lt.nsamp_step
        raw = synth.voltages(nblocks * step + lt.nsamp_overlap, freq, bw, tsamp, dm, period)
        d_raw = torch.from_numpy(raw).cuda()
        for b in range(nblocks):
            lt.process_block(d_raw[2 * b * step: 2 * (b * step + step + lt.nsamp_overlap)])
        lt.finish_subint()
        lt.synchronize()
        dumps.append([(s["hits"].copy(), s["profile_dev"].cpu().numpy()) for s in lt.subints])
        lt.close()
    assert len(dumps[0]) == len(dumps[1]) >= 1
    for (h0, p0), (h1, p1) in zip(*dumps):
        assert h0.sum() > 0 and np.abs(p0).max() > 0
        assert np.array_equal(h0, h1) and np.array_equal(p0, p1)
