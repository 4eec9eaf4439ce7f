"""GPU parity of the filterbank's input loaders at every address, layout and stride the C-ABI accepts.

dsp::TimeSeries places its rows at buffer + reserve_nfloat and seek() moves them by whole samples, so float32 rows start at any
4-byte boundary with any channel and polarisation strides; the raw side channel takes any BitSeries::get_rawptr(), so an 8-bit
block starts at any byte.  Pass 1 and the dispatcher (csrc/filterbank.hip fb_run) pick their loads from that address and those
strides.  Every case below names the branch it is there for: a condition of the dispatcher (a function or local of
filterbank.hip) or of a loader (file:line); blocks are placed by
test_gpu_parity._fb_case (offset / row_pad, sentinel guards around the block, outputs asserted finite) and compared with the
float64 oracle at the bounds of test_gpu_parity.py.  Only addresses whose alignment meets the width of the loads of the branch
they target are built: the byte and half-word branches take any byte offset, UWB blocks multiples of 4, CASPSR multiples of 2.
"""
import math

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


# ---- generic 8-bit blocks, multi-pass convolving filterbank ------------------------------------------------------------------
# (C, M, nfilt, npart, kwargs, offset): part steps 6880 (real, C=16 M=256), 3488 (complex, C=32 M=128) are multiples of 4
@pytest.mark.parametrize("C,M,nfilt,npart,kw,offset", [
    # real dual-pol, one channel: fb_common.h:339 (one 32-bit word, base & 3 == 0; fb_pass1 fast8 + k_raw_transpose),
    # fb_common.h:341 (half words, base & 1 == 0), fb_common.h:345 (bytes, odd base)
    (16, 256, (20, 21), 3, dict(max_parts=2), 0),
    (16, 256, (20, 21), 3, dict(max_parts=2), 1),
    (16, 256, (20, 21), 3, dict(max_parts=2), 2),
    (16, 256, (20, 21), 3, dict(max_parts=2), 3),
    (16, 256, (20, 21), 3, dict(max_parts=2), 4),
    # the same branches under the four-pass inverse (k_inv_a + k_inv_b)
    (16, 256, (20, 21), 3, dict(max_parts=2, four_pass=True), 1),
    (16, 256, (20, 21), 3, dict(max_parts=2, four_pass=True), 2),
    # two input channels: fb_common.h:341 (nchan != 1, even base) and :345 (odd base); fast8 off (input_nchan != 1)
    (16, 256, (20, 21), 2, dict(input_nchan=2), 0),
    (16, 256, (20, 21), 2, dict(input_nchan=2), 1),
    # real single-pol at an odd base: fb_common.h:347-349 (one byte per sample, stride skip)
    (16, 256, (20, 21), 2, dict(npol=1), 1),
    # complex dual-pol, one channel, logR = 5 >= 3: offset 0 fb_pass1 fastc (16-byte base, part step % 4 == 0:
    # k_raw_transpose); offset 8 fb_common.h:356 (the uint2 load, base & 7 == 0, polarisation picked at :405); offsets 4, 2
    # fb_common.h:361 (16-bit loads); offsets 1, 3 fb_common.h:365 (bytes)
    (32, 128, (9, 10), 2, dict(real=False), 0),
    (32, 128, (9, 10), 2, dict(real=False), 8),
    (32, 128, (9, 10), 2, dict(real=False), 4),
    (32, 128, (9, 10), 2, dict(real=False), 2),
    (32, 128, (9, 10), 2, dict(real=False), 1),
    (32, 128, (9, 10), 2, dict(real=False), 3),
    # complex, part step 4096 - 201 * 2 = 3694 = 2 (mod 4) on an aligned block: fb_pass1 fastc off, fb_common.h:356
    (2, 2048, (100, 101), 3, dict(real=False, max_parts=2), 0),
    # complex with 3 input channels: fb_common.h:361 (even base), :365 (odd base); the uint2 load needs one channel
    (32, 128, (9, 10), 2, dict(real=False, input_nchan=3), 0),
    (32, 128, (9, 10), 2, dict(real=False, input_nchan=3), 2),
    (32, 128, (9, 10), 2, dict(real=False, input_nchan=3), 1),
    # complex single-pol at an odd base: fb_common.h:365 (npol 1: no uint2 load at any address)
    (32, 128, (9, 10), 2, dict(real=False, npol=1), 1),
])
def test_generic_8bit_blocks_at_every_offset(oracle, gpu, C, M, nfilt, npart, kw, offset):
    _fb_case(oracle, gpu, C, M, nfilt, npart, offset=offset, **kw)


# ---- two-pass family of short responses (complex dual-pol, nchan_subband * freq_res^2 = 2^27) ----------------------------------
@pytest.mark.parametrize("input_nchan,offset", [
    (1, 0),     # fb_takes_two_pass: one input channel needs a 16-byte base (k_raw_cols' uint4 loads, fb_two_pass.hip:37)
    (1, 8),     # not 16-byte aligned: two and fastc off, the three-pass kernels with fb_common.h:356 (uint2 loads)
    (1, 1),     # the three-pass kernels with fb_common.h:365 (bytes)
    (2, 4),     # fb_takes_two_pass with k1c: several channels need a 4-byte base (fb_two_pass.hip:52, 32-bit loads)
    (2, 2),     # 2-byte base: two off, three-pass kernels with fb_common.h:361
])
def test_two_pass_family_at_offsets(oracle, gpu, input_nchan, offset):
    _fb_case(oracle, gpu, 512, 512, (27, 27), 2, npol=2, real=False, max_parts=2, input_nchan=input_nchan, offset=offset)


# ---- odd factors: nchan_subband = 3 * 2^k (k_sub_split de-interleaves the shifted block), freq_res = 3 * 2^k -------------------
@pytest.mark.parametrize("C,M,offset", [
    (96, 256, 1),       # fb_fwd_cols.hip sub_split_load<1, 2>: odd element address, byte loads
    (96, 256, 2),       # even address: 16-bit loads, the fast form off (the element address is not 4-byte aligned)
    (16, 768, 3),       # freq_res = 3 * 256: k_sub_split with R = 3 on an odd block, then k_time_combine
])
def test_odd_factors_on_shifted_blocks(oracle, gpu, C, M, offset):
    _fb_case(oracle, gpu, C, M, (20, 21), 3, max_parts=2, offset=offset)


def test_odd_factor_complex_float_rows_at_odd_offsets(oracle, gpu):
    # fb_fwd_cols.hip sub_split_load<0, 8>: complex float rows at an odd float offset / with odd strides take two 4-byte loads
    # (an 8-byte load there would be misaligned)
    for offset, row_pad in [(1, 0), (0, 1)]:
        _fb_case(oracle, gpu, 48, 128, (9, 10), 2, real=False, use_raw=False, offset=offset, row_pad=row_pad)


# ---- CASPSR ---------------------------------------------------------------------------------------------------------------
def test_caspsr_block_at_a_group_boundary_not_16_byte_aligned(oracle, gpu):
    # offset 8: fb_pass1 fast8 (base % 4 == 0) with k_raw_transpose's CASPSR 32-bit loads (fb_fwd_cols.hip:45)
    _fb_case(oracle, gpu, 16, 256, (20, 21), 3, layout="caspsr", max_parts=2, offset=8)
    # offset 2: fast8 off, fb_common.h:325 (16-bit loads)
    _fb_case(oracle, gpu, 16, 256, (20, 21), 3, layout="caspsr", max_parts=2, offset=2)


def test_caspsr_part_step_not_a_multiple_of_4(oracle, gpu):
    # C = 1 real, nfilt sum 601: part step 2 * (4096 - 601) = 6990 = 2 (mod 4): fb_pass1 turns the regroup off
    _fb_case(oracle, gpu, 1, 4096, (300, 301), 3, layout="caspsr", max_parts=2)


def test_odd_caspsr_and_uwb_addresses_are_refused(oracle, gpu):
    """filterbank.hip fb_run: a CASPSR block at an odd address or a UWB block off a 4-byte boundary would take misaligned 16 / 32-bit
    loads; refused with DSPSR_AMD_EINVAL before any launch."""
    dspsr_amd, ctx = gpu
    b = _fb_block(oracle, gpu, 16, 256, (20, 21), 2, layout="caspsr", offset=1)
    out = torch.full((16, 2, 2 * 2 * b.plan.nkeep), -3.0, dtype=torch.float32, device="cuda")
    with pytest.raises(dspsr_amd.DspsrAmdError, match="multiple of 2 bytes"):
        b.eng.perform_raw(b.raw, b.layout, b.scale, out, 2)
    b.eng.close()
    b = _fb_block(oracle, gpu, 8, 256, (30, 31), 2, real=False, layout="uwb16")
    shifted = b.raw[2:]
    for run in (lambda: b.eng.perform_raw(shifted, b.layout, 1.0, out, 2),
                lambda: b.eng.perform_detect(torch.zeros((8, 1, 4 * 2 * b.plan.nkeep), device="cuda"), 2, raw=shifted, layout=b.layout)):
        with pytest.raises(dspsr_amd.DspsrAmdError, match="multiple of 4 bytes"):
            run()
    b.eng.finish()
    b.eng.close()
    assert (out == -3.0).all()


# ---- 16-bit UWB blocks in every family that takes them -------------------------------------------------------------------
# part steps that are not multiples of 2048 and enough parts to cross at least three 2048-sample blocks; fb_common.h:329 reads t and
# t + 1 through their own block indices
@pytest.mark.parametrize("C,M,nfilt,npart,npol,kw,offset", [
    (8, 256, (30, 31), 5, 2, dict(max_parts=2), 0),                 # three-pass, part step 1560
    (8, 256, (30, 31), 5, 2, dict(max_parts=2), 4),
    (8, 256, (30, 31), 5, 1, dict(max_parts=3), 12),
    (8, 256, (30, 31), 5, 2, dict(max_parts=2, four_pass=True), 4),  # four-pass (forced)
    (4, 16384, (900, 1100), 2, 2, dict(max_parts=2), 0),            # four-pass by length (freq_res > 8192), part step 57536
    (512, 512, (27, 27), 2, 2, dict(max_parts=2), 0),               # the two-pass geometry: fb_takes_two_pass needs kind 1,
                                                                    # so UWB takes the three-pass kernels; part step 234496
    (1, 4096, (300, 301), 3, 2, dict(max_parts=2), 4),              # a conv1 object (nchan_subband 1, M <= 2^13): fb_run conv_rows
                                                                    # needs float rows, raw input falls back; part step 3495
    (1, 32768, (3000, 2000), 2, 2, dict(max_parts=2), 0),           # a conv3 object (fb_run conv_rows), part step 27768
])
def test_uwb16_blocks_in_every_family(oracle, gpu, C, M, nfilt, npart, npol, kw, offset):
    _fb_case(oracle, gpu, C, M, nfilt, npart, npol=npol, real=False, layout="uwb16", offset=offset, **kw)


@pytest.mark.parametrize("C,npart", [(64, 120), (1024, 7), (4096, 3)])
@pytest.mark.parametrize("npol", [1, 2])
def test_uwb16_non_convolving(oracle, gpu, C, npart, npol):
    # fb_plain.hip:83 F_UWB (MODE 2); part step C: 4096 is a whole block, the others are not; every case crosses >= 3 blocks
    _fb_case(oracle, gpu, C, 1, (0, 0), npart, npol=npol, real=False, layout="uwb16", offset=4)


def test_uwb16_odd_factor_is_refused(oracle, gpu):
    """filterbank.hip fb_run_subbands: k_sub_split de-interleaves 8-bit and float32 input only."""
    dspsr_amd, ctx = gpu
    b = _fb_block(oracle, gpu, 96, 256, (20, 21), 2, real=False, layout="uwb16")
    out = torch.full((96, 2, 2 * 2 * b.plan.nkeep), -3.0, dtype=torch.float32, device="cuda")
    with pytest.raises(dspsr_amd.DspsrAmdError, match="16-bit UWB blocks need power-of-two"):
        b.eng.perform_raw(b.raw, b.layout, 1.0, out, 2)
    b.eng.finish()
    b.eng.close()
    assert (out == -3.0).all()


# ---- k_fb_plain input forms (freq_res = 1) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,npart,kw,offset", [
    (64, 90, dict(input_nchan=3), 0),          # fb_plain.hip:81 F_BYTES (MODE 0): several input channels
    (64, 90, dict(), 1),                       # F_BYTES: one channel, base & 3 != 0
    (64, 90, dict(), 2),
    (64, 130, dict(npol=1), 0),                # fb_plain.hip:82 MODE 1 raw: F_BYTES at every address
    (64, 130, dict(npol=1), 1),
    (128, 67, dict(real=False), 0),            # fb_plain.hip:83 F_HALF: complex 8-bit, even base
    (128, 67, dict(real=False), 2),
    (128, 67, dict(real=False), 1),            # F_BYTES complex: odd base
    (128, 67, dict(real=False), 3),
    (128, 67, dict(real=False, npol=1), 2),    # F_HALF with one polarisation (consecutive parts per column pair)
    (2048, 5, dict(), 1),                      # MODE 3 (fb_plain.hip:434 plain_pol_split: real dual-pol, C >= 2048, complex output)
                                               # with F_BYTES (fb_plain.hip:166)
    (8192, 3, dict(), 3),
    (256, 37, dict(), 1),                      # F_BYTES either side of the tile switch (fb_plain.hip:48: 2^13 points up to 256
    (512, 9, dict(), 1),                       # channels, 2^14 above)
    (256, 37, dict(real=False), 1),
    (512, 9, dict(real=False), 1),
])
def test_plain_filterbank_input_forms(oracle, gpu, C, npart, kw, offset):
    _fb_case(oracle, gpu, C, 1, (0, 0), npart, offset=offset, **kw)


# ---- float32 rows at odd addresses and strides ------------------------------------------------------------------------------
# Each object is run on aligned rows and on rows shifted by 1-3 floats or padded by one float per row (odd channel and
# polarisation strides); the shifted runs must meet the oracle and equal the aligned run to the bound of
# test_filterbank_float_input_equals_raw.
FLOAT_OBJECTS = {
    # fb_run conv_rows (conv1) needs an 8-byte base and even strides: shifted rows fall back to the multi-pass kernels
    "conv1": (1, 4096, (300, 301), 3, dict(real=False, max_parts=2)),
    "conv1_3ch": (1, 4096, (300, 301), 2, dict(real=False, input_nchan=3, max_parts=2)),
    # fb_run conv_rows (conv3, M = 2^15): the same conditions
    "conv3": (1, 32768, (3000, 2000), 2, dict(real=False, max_parts=2)),
    # fb_run batch -> fb_run_batched (input_nchan 4, the four-pass kernels) needs an even channel stride, which two polarisation rows
    # keep under row_pad 1; its pass 1 reads 4-byte words, so shifted rows and odd polarisation strides stay on this path
    "batch": (1, 1024, (100, 90), 3, dict(real=False, input_nchan=4, max_parts=2, four_pass=True)),
    # fb_pass1 FB_REGROUP_FLOAT (logR >= 6, 1 <= logT1 <= 4): a 16-byte base and strides % 4 == 0
    "pretf": (64, 1024, (100, 101), 2, dict(max_parts=2)),
    # fb_plain.hip F_FLOAT: scalar loads at any float address
    "plain": (128, 1, (0, 0), 70, dict()),
}


@pytest.mark.parametrize("offset,row_pad", [(1, 0), (2, 0), (3, 0), (0, 1)])
@pytest.mark.parametrize("obj", sorted(FLOAT_OBJECTS))
def test_float_rows_at_odd_offsets_and_strides(oracle, gpu, obj, offset, row_pad):
    C, M, nfilt, npart, kw = FLOAT_OBJECTS[obj]
    a, _ = _fb_case(oracle, gpu, C, M, nfilt, npart, use_raw=False, **kw)
    b, _ = _fb_case(oracle, gpu, C, M, nfilt, npart, use_raw=False, offset=offset, row_pad=row_pad, **kw)
    assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max()


# ---- epilogues on shifted and UWB blocks ----------------------------------------------------------------------------------
EPILOGUE_CASES = {
    "generic_offset1": (16, 256, (20, 21), 4, dict(max_parts=2, offset=1)),                     # fb_common.h:345
    "complex_offset2": (32, 128, (9, 10), 4, dict(real=False, max_parts=2, offset=2)),          # fb_common.h:361
    "uwb16": (8, 256, (30, 31), 5, dict(real=False, layout="uwb16", max_parts=2, offset=4)),    # fb_common.h:329
}


@pytest.mark.parametrize("state", ["Coherence", "Stokes"])
@pytest.mark.parametrize("case", sorted(EPILOGUE_CASES))
def test_detect_on_shifted_blocks(oracle, gpu, case, state):
    """perform_detect (ndim 4) == Detection::polarimetry of the float64 filterbank to 1e-5 of the largest value."""
    dspsr_amd, ctx = gpu
    C, M, nfilt, npart, kw = EPILOGUE_CASES[case]
    b = _fb_block(oracle, gpu, C, M, nfilt, npart, **kw)
    want = oracle.detect_layout(oracle.detect_products(b.ref, state), 4)
    det = torch.full((b.nchan, 1, 4 * npart * b.plan.nkeep), float("nan"), dtype=torch.float32, device="cuda")
    b.eng.perform_detect(det, npart, dspsr_amd.STOKES if state == "Stokes" else dspsr_amd.COHERENCE, 4, raw=b.raw, layout=b.layout,
                         scale=b.scale)
    b.eng.finish()
    got = det.cpu().numpy().reshape(want.shape)
    b.eng.close()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("case", sorted(EPILOGUE_CASES))
def test_fold_on_shifted_blocks(oracle, gpu, case):
    """perform_fold (FUSED_ALWAYS) == perform_detect + FoldEngine.fold: bit for bit where the fold is not segmented
    (test_fused_fold_bit_identical), to float rounding where it is."""
    dspsr_amd, ctx = gpu
    C, M, nfilt, npart, kw = EPILOGUE_CASES[case]
    b = _fb_block(oracle, gpu, C, M, nfilt, npart, fused_fold=dspsr_amd.FUSED_ALWAYS, **kw)
    fused = b.eng.fold_is_fused()
    nbin, pps = 100, 1.0 / 97.3
    ndat = npart * b.plan.nkeep
    folds, hits = [dspsr_amd.FoldEngine(ctx), dspsr_amd.FoldEngine(ctx)], [np.zeros(nbin, np.uint32), np.zeros(nbin, np.uint32)]
    for f, h in zip(folds, hits):
        f.set_shape(b.nchan, 1, 4, nbin)
        f.set_nbin(nbin)
        f.set_ndat(ndat, 0)
        f.set_bins(0.37, pps, ndat, 0, h)
    det = torch.zeros((b.nchan, 1, 4 * ndat), dtype=torch.float32, device="cuda")
    b.eng.perform_detect(det, npart, dspsr_amd.COHERENCE, 4, raw=b.raw, layout=b.layout, scale=b.scale)
    folds[0].fold(det)
    b.eng.perform_fold(folds[1], npart, dspsr_amd.COHERENCE, raw=b.raw, layout=b.layout, scale=b.scale)
    x, y = folds[0].synch(), folds[1].synch()
    b.eng.close()
    for f in folds:
        f.close()
    assert np.array_equal(hits[0], hits[1]) and np.isfinite(y).all() and np.abs(x).max() > 0
    if fused != 2:
        assert np.array_equal(x, y)
    else:                                           # parts cut into runs: sums re-associated (test_gpu_parity.py, segmented fold)
        assert np.abs(x - y).max() <= 2e-6 * np.abs(x).max()


@pytest.mark.parametrize("case", sorted(EPILOGUE_CASES))
def test_search_on_shifted_blocks(oracle, gpu, case):
    """perform_search (Intensity, tscrunch 3) == square_law + tscrunch_fpt of the same object's perform_raw output, bit for bit
    (the pattern of tests/test_gpu_search.py)."""
    dspsr_amd, ctx = gpu
    C, M, nfilt, npart, kw = EPILOGUE_CASES[case]
    b = _fb_block(oracle, gpu, C, M, nfilt, npart, **kw)
    sf = 3
    cplx = torch.zeros((b.nchan, 2, 2 * npart * b.plan.nkeep), dtype=torch.float32, device="cuda")
    b.eng.perform_raw(b.raw, b.layout, b.scale, cplx, npart)
    want = oracle.tscrunch_fpt(oracle.square_law(cplx.cpu().numpy().view(np.complex64), "Intensity"), sf)
    carry = torch.zeros((b.nchan, 1), dtype=torch.float32, device="cuda")
    out = torch.full((b.nchan, 1, npart * b.plan.nkeep // sf + 1), -1.0, dtype=torch.float32, device="cuda")
    nout, cc = b.eng.perform_search(out, carry, 0, npart, sf, dspsr_amd.INTENSITY, raw=b.raw, layout=b.layout, scale=b.scale)
    b.eng.finish()
    got = out[:, :, :nout].cpu().numpy()
    b.eng.close()
    assert (nout, cc) == (npart * b.plan.nkeep // sf, npart * b.plan.nkeep % sf)
    assert got.shape == want.shape and np.array_equal(got, want)
    # (the filterbank output itself met the oracle in the case's own parity test above)
    assert math.isfinite(float(np.abs(got).max()))
