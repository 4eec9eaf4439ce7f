"""The matrix response of the filterbank (`dspsr -pac`, dspsr_amd_filterbank_set_response_matrix; csrc/fb_inv_chan.h FB_EPI_MATRIX).

Reference: tests/matrix_cases.py filterbank_matrix in float64 -- Filterbank.C:561-662 with Response::operate(data1, data2)
(Response.C:515-585) -- and the project's filterbank bound (test_gpu_parity._fb_case): rms(err) / rms(out) <= tol =
2e-6 * sqrt(log2(2 C M)), max |err| <= 8 tol rms(out).  The response of a case is one independent Jones matrix per bin
(U diag(g1, g2) V, condition number <= 4) times a random-phase chirp with bin 0 zeroed.

Shapes: those of tests/test_gpu_presplit.py (its docstring says which branch of the passes each reaches).  The float64 reference
and the default-path output of a case are computed once per module and shared."""
import numpy as np
import pytest

import matrix_cases as mc
from device_buffers import OutputLayout, SENTINEL, sentinel_rows, written_mask

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


_RESPONSES = {}


def response_of(n):
    if n not in _RESPONSES:
        _RESPONSES[n] = mc.matrix_response(n)
    return _RESPONSES[n]


def run_matrix(oracle, gpu, C, M, nfilt, npart, max_parts, kw, response=None, **setup):
    """(output complex64, block) of a case with its matrix response on an object built with `setup`"""
    b = mc.device_block(oracle, gpu, torch, C, M, nfilt, npart, max_parts=max_parts, **kw, **setup)
    b.eng.set_response_matrix(response_of(C * M) if response is None else response)
    assert b.eng.response_ndim() == 8 and b.eng.npass(True) == 3 and b.eng.npass(False) == 3
    assert b.eng.fold_is_fused() == 0 and not b.eng.search_is_fused()
    return mc.run_complex(b, torch), b


def case_id(c):
    return "%dx%d%s" % (c[0], c[1], "" if not c[5] else "-" + "-".join("%s=%s" % kv for kv in sorted(c[5].items())))


@pytest.mark.parametrize("case", mc.REAL_CASES, ids=case_id)
def test_parity_and_split_placement_real_input(oracle, gpu, case):
    """Real input: the default object (pre-split spectrum) and split_in_inverse = 1 give the same bits, within the bound of the
    float64 restatement."""
    C, M, nfilt, npart, max_parts, kw = case
    got, b = run_matrix(oracle, gpu, C, M, nfilt, npart, max_parts, kw)
    assert b.eng.presplit() is True
    b.eng.close()
    old, b2 = run_matrix(oracle, gpu, C, M, nfilt, npart, max_parts, kw, split_in_inverse=True)
    assert b2.eng.presplit() is False
    b2.eng.close()
    assert np.array_equal(got, old), "the pre-split form and the split in the inverse pass differ"
    ref = mc.filterbank_matrix(b.unpacked, b.plan, response_of(C * M), npart, dtype=np.float64)
    mc.assert_fb_bound(got, ref, C, M)


def test_parity_complex_input(oracle, gpu):
    C, M, nfilt, npart, max_parts, kw = mc.COMPLEX_CASE
    got, b = run_matrix(oracle, gpu, C, M, nfilt, npart, max_parts, kw)
    assert b.eng.presplit() is False
    b.eng.close()
    ref = mc.filterbank_matrix(b.unpacked, b.plan, response_of(C * M), npart, dtype=np.float64)
    mc.assert_fb_bound(got, ref, C, M)


def test_two_pass_geometry_takes_three_passes(oracle, gpu):
    C, M, nfilt, npart, max_parts, kw = mc.TWO_PASS_CASE
    b = mc.device_block(oracle, gpu, torch, C, M, nfilt, npart, max_parts=max_parts, **kw)
    assert b.eng.npass(True) == 2, "the geometry must be one of the two-pass path"
    b.eng.set_response_matrix(response_of(C * M))
    assert b.eng.npass(True) == 3
    got = mc.run_complex(b, torch)
    b.eng.close()
    ref = mc.filterbank_matrix(b.unpacked, b.plan, response_of(C * M), npart, dtype=np.float64)
    mc.assert_fb_bound(got, ref, C, M)


@pytest.mark.parametrize("split_in_inverse", [False, True], ids=["presplit", "split_in_inverse"])
@pytest.mark.parametrize("real", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("C,M,nfilt", [(16, 256, (20, 21)), (4, 4096, (422, 422))])
def test_diagonal_response_equals_the_scalar_response(oracle, gpu, C, M, nfilt, real, split_in_inverse):
    """diag(k, k) adds 0 * d through an fma onto the scalar path's complex multiply: the same bits as set_kernel(k).
    (Complex 8-bit input at (4, 4096) is a geometry of the two-pass path, whose transforms are factored differently -- 1e-7
    apart, never bit-equal to the three passes: force_four_pass = 2 keeps the scalar response on the three passes the matrix
    response takes, so that the two runs differ in the response multiply alone.)"""
    dspsr_amd, _ = gpu
    k = mc.random_chirp(C * M)
    b = mc.device_block(oracle, gpu, torch, C, M, nfilt, 2, real=real, max_parts=2, fused_fold=dspsr_amd.FUSED_NEVER,
                        split_in_inverse=split_in_inverse, force_four_pass=0 if real else 2)
    assert b.eng.presplit() is (real and not split_in_inverse) and b.eng.npass(True) == 3
    b.eng.set_kernel(k)
    scalar = mc.run_complex(b, torch).copy()
    b.eng.set_response_matrix(mc.diagonal_response(k))
    assert b.eng.response_ndim() == 8
    matrix = mc.run_complex(b, torch)
    b.eng.close()
    assert np.abs(scalar).max() > 0
    assert np.array_equal(scalar, matrix)


def test_setting_order(oracle, gpu):
    """set_kernel after set_response_matrix and the reverse give what the last call set; response_ndim says 8, 2, 0"""
    C, M, nfilt = 16, 256, (20, 21)
    k = mc.random_chirp(C * M, seed=8)
    b = mc.device_block(oracle, gpu, torch, C, M, nfilt, 2, max_parts=2)
    assert b.eng.response_ndim() == 0
    b.eng.set_kernel(k)
    want_scalar = mc.run_complex(b, torch).copy()
    b.eng.set_response_matrix(response_of(C * M))
    assert b.eng.response_ndim() == 8
    want_matrix = mc.run_complex(b, torch).copy()
    assert not np.array_equal(want_scalar, want_matrix)
    b.eng.set_kernel(k)
    assert b.eng.response_ndim() == 2
    assert np.array_equal(mc.run_complex(b, torch), want_scalar)
    b.eng.set_response_matrix(response_of(C * M))
    assert b.eng.response_ndim() == 8
    assert np.array_equal(mc.run_complex(b, torch), want_matrix)
    b.eng.set_kernel(None)
    assert b.eng.response_ndim() == 0
    plain = mc.run_complex(b, torch).copy()
    b.eng.close()
    b2 = mc.device_block(oracle, gpu, torch, C, M, nfilt, 2, max_parts=2)
    assert np.array_equal(mc.run_complex(b2, torch), plain), "set_kernel(NULL) must clear a matrix response"
    b2.eng.close()


@pytest.mark.parametrize("C,M,nfilt", [(1024, 16, (1, 2)), (16, 256, (20, 21))])
def test_launch_groups(oracle, gpu, C, M, nfilt):
    """5 parts in groups of four and one equal the same block in one group of 5, bit for bit"""
    a, b1 = run_matrix(oracle, gpu, C, M, nfilt, 5, 4, {})
    b1.eng.close()
    b, b2 = run_matrix(oracle, gpu, C, M, nfilt, 5, 5, {})
    b2.eng.close()
    assert np.abs(a).max() > 0 and np.array_equal(a, b)


@pytest.fixture(scope="module", params=[(16, 256, (20, 21)), (4, 4096, (422, 422))], ids=["16x256", "4x4096"])
def outputs_block(request, oracle, gpu):
    """an object with its matrix response and its own complex output (three parts in groups of two and one)"""
    C, M, nfilt = request.param
    got, b = run_matrix(oracle, gpu, C, M, nfilt, 3, 2, {})
    b.complex = got.copy()
    yield b
    b.eng.close()


@pytest.mark.parametrize("ndim", [1, 2, 4])
@pytest.mark.parametrize("state", ["Coherence", "Stokes"])
def test_detected_output(oracle, gpu, outputs_block, state, ndim):
    """perform_detect equals Detection of the object's own complex output (rtol 3e-7: the bound of the existing detection tests)"""
    dspsr_amd, _ = gpu
    b = outputs_block
    n = b.npart * b.plan.nkeep
    det = torch.zeros((b.C, 4 // ndim, n * ndim), dtype=torch.float32, device="cuda")
    b.eng.perform_detect(det, b.npart, dspsr_amd.COHERENCE if state == "Coherence" else dspsr_amd.STOKES, ndim, raw=b.raw,
                         layout=b.layout, scale=b.scale)
    b.eng.finish()
    want = oracle.detect_layout(oracle.detect_products(b.complex, state), ndim)
    assert det.numel() == want.size
    got = det.cpu().numpy().reshape(want.shape)
    np.testing.assert_allclose(got, want, rtol=3e-7, atol=3e-7 * np.abs(want).max())


def test_fold_runs_through_the_detected_block(oracle, gpu, outputs_block):
    dspsr_amd, ctx = gpu
    b = outputs_block
    nbin, n = 32, b.npart * b.plan.nkeep
    assert b.eng.fold_is_fused() == 0
    det = torch.zeros((b.C, 1, 4 * n), dtype=torch.float32, device="cuda")
    b.eng.perform_detect(det, b.npart, dspsr_amd.COHERENCE, 4, raw=b.raw, layout=b.layout, scale=b.scale)
    profiles = []
    for fused in (False, True):
        fold = dspsr_amd.FoldEngine(ctx)
        fold.set_shape(b.C, 1, 4, nbin)
        fold.set_nbin(nbin)
        fold.set_ndat(n, 0)
        fold.set_bins(0.123, 1.0 / 77.7, n, 0, np.zeros(nbin, np.uint32))
        if fused:
            b.eng.perform_fold(fold, b.npart, dspsr_amd.COHERENCE, raw=b.raw, layout=b.layout, scale=b.scale)
        else:
            fold.fold(det)
        profiles.append(fold.synch().copy())
        fold.close()
    assert np.abs(profiles[0]).max() > 0
    assert np.array_equal(profiles[0], profiles[1])


def test_search_runs_through_the_detected_block(oracle, gpu, outputs_block):
    dspsr_amd, ctx = gpu
    b = outputs_block
    sf, n = 4, b.npart * b.plan.nkeep
    assert not b.eng.search_is_fused()
    nout_max = n // sf + 1
    out = torch.zeros((b.C, 1, nout_max), dtype=torch.float32, device="cuda")
    carry = torch.zeros((b.C, 1), dtype=torch.float32, device="cuda")
    nout, cc = b.eng.perform_search(out, carry, 0, b.npart, sf, dspsr_amd.INTENSITY, raw=b.raw, layout=b.layout, scale=b.scale)
    b.eng.finish()
    # the same from the pieces: complex rows -> square law (Intensity) -> time scrunch
    cplx = torch.zeros((b.C, 2, 2 * n), dtype=torch.float32, device="cuda")
    b.eng.perform_raw(b.raw, b.layout, b.scale, cplx, b.npart)
    det = torch.zeros((b.C, 1, n), dtype=torch.float32, device="cuda")
    dspsr_amd.DetectionEngine(ctx).square_law(cplx, det, True)
    out2 = torch.zeros_like(out)
    carry2 = torch.zeros_like(carry)
    nout2, cc2 = dspsr_amd.tscrunch_fpt(ctx, det, out2, sf, carry2, 0)
    ctx.synchronize()
    assert (nout, cc) == (nout2, cc2) == (n // sf, n % sf) and nout > 0
    assert np.abs(out.cpu().numpy()).max() > 0
    assert np.array_equal(out.cpu().numpy(), out2.cpu().numpy()) and np.array_equal(carry.cpu().numpy(), carry2.cpu().numpy())


REFUSALS = {
    # name: (C, M, nfilt, setup keywords, matrices handed in (None: C * M), scalar kernel bins for the call afterwards)
    "freq_res_1": (64, 1, (0, 0), {}, None),
    "freq_res_16384": (2, 16384, (900, 1100), {}, None),
    "nchan_subband_1": (1, 4096, (300, 301), dict(real_input=False), None),
    "nchan_subband_96": (96, 256, (20, 21), {}, None),
    "npol_1": (16, 256, (20, 21), dict(npol=1), None),
    "input_nchan_2": (16, 256, (20, 21), dict(input_nchan=2), None),
    "wrong_nmatrix": (16, 256, (20, 21), {}, 16 * 256 - 1),
    "force_four_pass": (16, 256, (20, 21), dict(force_four_pass=1), None),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(oracle, gpu, name):
    """EINVAL with a message naming the limit; the object then still performs with a scalar kernel"""
    dspsr_amd, ctx = gpu
    C, M, nfilt, kw, nmatrix = REFUSALS[name]
    kw = dict(kw)
    input_nchan, npol, real = kw.pop("input_nchan", 1), kw.pop("npol", 2), kw.pop("real_input", True)
    eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, nfilt[0], nfilt[1], input_nchan, npol, real, None, max_parts=2, **kw)
    n = C * M if nmatrix is None else nmatrix
    zeros = np.zeros((n, 8), np.float32)
    rc = dspsr_amd.lib.dspsr_amd_filterbank_set_response_matrix(eng.handle, zeros.ctypes.data, n)
    assert rc == -1, "DSPSR_AMD_EINVAL expected, got %d" % rc          # include/dspsr_amd.h: DSPSR_AMD_EINVAL
    msg = dspsr_amd.lib.dspsr_amd_last_error(ctx.handle).decode()
    assert msg, "a refusal must leave a message"
    print(name, "->", msg)
    assert eng.response_ndim() == 0
    # ... and still runs with a scalar kernel: two parts of zeros in, finite numbers out
    eng.set_kernel(mc.random_chirp(input_nchan * C * M))
    assert eng.response_ndim() == 2
    ndim = 1 if real else 2
    raw = torch.zeros(((2 * eng.nsamp_step + eng.nsamp_overlap) * input_nchan * npol * ndim,), dtype=torch.int8, device="cuda")
    out = torch.zeros((input_nchan * C, npol, 2 * 2 * eng.nkeep), dtype=torch.float32, device="cuda")
    eng.perform_raw(raw, dspsr_amd.RAW_GENERIC, 1.0, out, 2)
    eng.finish()
    assert np.isfinite(out.cpu().numpy()).all()
    eng.close()


def test_writer_touches_only_the_output_rows(oracle, gpu):
    """complex rows cut from a sentinel buffer (float-aligned rows, padded strides, parts further apart than 2 * nkeep)"""
    C, M, nfilt, npart = 16, 256, (20, 21), 3
    b = mc.device_block(oracle, gpu, torch, C, M, nfilt, npart, max_parts=2)
    b.eng.set_response_matrix(response_of(C * M))
    want = mc.run_complex(b, torch).copy()
    nkeep, step = b.plan.nkeep, 2 * b.plan.nkeep + 6
    lay = OutputLayout(C, 2, (npart - 1) * step + 2 * nkeep, 1, 3)
    buf, rows = sentinel_rows(lay)
    b.eng.perform_raw(b.raw, b.layout, b.scale, rows, npart, out_step=step)
    b.eng.finish()
    b.eng.close()
    bits = buf.cpu().numpy()
    mask = written_mask(lay, npart, step, 2 * nkeep)
    assert (bits[~mask] == SENTINEL).all(), "floats outside the output rows were written"
    got = rows.cpu().numpy()
    for p in range(npart):
        part = np.ascontiguousarray(got[:, :, p * step:p * step + 2 * nkeep]).view(np.complex64)
        assert np.array_equal(part, want[:, :, p * nkeep:(p + 1) * nkeep])
