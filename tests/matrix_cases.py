"""Helpers of the matrix-response tests (no test here): a numpy restatement of the filterbank with the matrix branch, a seeded
Jones generator, the device block of a case and the case list.

filterbank_matrix restates dsp::Filterbank::filterbank (Filterbank.C:561-662) where `matrix_convolution` holds (:574-656): both
polarisations of a part are transformed first, Response::operate(data1, data2) (Response.C:515-585) multiplies the pair of
spectra by the bin's Jones matrix, then both are transformed back.  The oracle's filterbank() is the scalar branch and stays
as it is."""
import math
import types

import numpy as np

# (C, M, nfilt, npart, max_parts, keywords of the block): the geometries of tests/test_gpu_presplit.py, whose docstring says which
# branch of the passes each reaches
REAL_CASES = [
    (1024, 16, (1, 2), 2, 1, {}),
    (4096, 16, (1, 2), 2, 1, {}),
    (16, 256, (20, 21), 2, 1, {}),
    (4, 4096, (422, 422), 2, 1, {}),
    (1024, 4096, (843, 844), 2, 2, {}),                  # the full-tile instantiations
    (2048, 16, (1, 2), 2, 2, dict(use_raw=False)),       # float32 rows
]
COMPLEX_CASE = (32, 128, (9, 10), 3, 2, dict(real=False))
# a geometry of the two-pass path (complex dual-pol 8-bit input): the row (16, 512, (40, 3)) of tests/test_gpu_two_pass.py -- ONE tile of
# Fb = 16 channels, N = 2^13, the smallest transform and float64 reference of that file's rows
TWO_PASS_CASE = (16, 512, (40, 3), 3, 2, dict(real=False))


def fb_tolerance(C, M):
    """the project's filterbank bound (test_gpu_parity._fb_case): rms(err) / rms(out) <= tol, max |err| <= 8 tol rms(out)"""
    return 2e-6 * math.sqrt(math.log2(2 * C * M))


def assert_fb_bound(got, ref, C, M):
    err = got.astype(np.complex128) - ref
    rms_ref = math.sqrt(np.mean(np.abs(ref) ** 2))
    rms_err = math.sqrt(np.mean(np.abs(err) ** 2))
    tol = fb_tolerance(C, M)
    print("matrix filterbank C=%d M=%d: rms %.3g (tol %.3g), max %.3g rms (bound %.3g)"
          % (C, M, rms_err / rms_ref, tol, np.abs(err).max() / rms_ref, 8 * tol))
    assert rms_ref > 0
    assert rms_err / rms_ref <= tol, (rms_err / rms_ref, tol)
    assert np.abs(err).max() <= 8 * tol * rms_ref, (np.abs(err).max() / rms_ref, 8 * tol)


def operate_matrix(d1, d2, m8):
    """Response::operate(data1, data2), Response.C:543-584, in the precision of the arguments: returns (d1', d2')."""
    f = [m8[:, 2 * e] + 1j * m8[:, 2 * e + 1] for e in range(4)]            # f11, f21, f22, f12
    rdt = d1.real.dtype
    if rdt == np.float32:
        # every product and sum in float32, in the order the reference writes them
        def parts(z):
            return z.real.astype(np.float32), z.imag.astype(np.float32)

        def mul(fz, dz):
            fr, fi = parts(fz)
            dr, di = parts(dz)
            return fr * dr - fi * di, fi * dr + fr * di

        def muladd(r, fz, dz):
            fr, fi = parts(fz)
            dr, di = parts(dz)
            return r[0] + fr * dr - fi * di, r[1] + fi * dr + fr * di
        r1, r2 = mul(f[0], d1), mul(f[1], d1)
        n2, n1 = muladd(r2, f[2], d2), muladd(r1, f[3], d2)
        return (n1[0] + 1j * n1[1]).astype(np.complex64), (n2[0] + 1j * n2[1]).astype(np.complex64)
    f = [x.astype(np.complex128) for x in f]
    r1, r2 = f[0] * d1, f[1] * d1
    return r1 + f[3] * d2, r2 + f[2] * d2


def filterbank_matrix(unpacked, plan, matrix8, npart, dtype=np.float32):
    """unpacked: float [1][2][ndat * ndim]; matrix8: float32 [N][8] (f11, f21, f22, f12 per bin) -> complex [C][2][npart * nkeep]"""
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    input_nchan, npol, _ = unpacked.shape
    assert input_nchan == 1 and npol == 2, "matrix convolution: one input channel (Filterbank.C:199-201), two polarisations"
    ndim = 1 if plan.real_input else 2
    N, M, C = plan.n_fft, plan.freq_res, plan.nchan_subband
    assert matrix8.shape == (N, 8)
    m8 = matrix8.astype(dtype)
    out = np.zeros((C, 2, npart * plan.nkeep), dtype=cdt)
    in_step = plan.nsamp_step * ndim
    for ipart in range(npart):
        spec = []
        for ipol in range(2):                                                # :574-595 both polarisations forward first
            x = unpacked[0, ipol, ipart * in_step: ipart * in_step + plan.nsamp_fft * ndim].astype(dtype)
            s = np.fft.rfft(x)[:N] if plan.real_input else np.fft.fft(x.view(cdt))
            spec.append(s.astype(cdt))
        d1, d2 = operate_matrix(spec[0], spec[1], m8)                        # :606-609
        for ipol, d in enumerate((d1, d2)):                                  # :640-652 unnormalised backward transforms
            t = (np.fft.ifft(d.astype(cdt).reshape(C, M), axis=1) * M).astype(cdt)
            out[:, ipol, ipart * plan.nkeep:(ipart + 1) * plan.nkeep] = t[:, plan.nfilt_pos: plan.nfilt_pos + plan.nkeep]
    return out


def _unitary(rng, n):
    th = rng.uniform(0.0, 0.5 * np.pi, n)
    a = np.cos(th) * np.exp(1j * rng.uniform(-np.pi, np.pi, n))
    b = np.sin(th) * np.exp(1j * rng.uniform(-np.pi, np.pi, n))
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi, n))
    u = np.empty((n, 2, 2), dtype=np.complex128)
    u[:, 0, 0], u[:, 0, 1], u[:, 1, 0], u[:, 1, 1] = a, b, -ph * np.conj(b), ph * np.conj(a)
    return u


def jones_matrices(n, seed=11):
    """n independent matrices U diag(g1, g2) V with U, V random unitary and g in [0.5, 2]: condition number <= 4"""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 2.0, (n, 2))
    u, v = _unitary(rng, n), _unitary(rng, n)
    return np.einsum("nij,nj,njk->nik", u, g.astype(np.complex128), v)


def pack8(jones):
    """[n][2][2] complex -> float32 [n][8] in the reference's order f11, f21, f22, f12 (Response.C:614-640)"""
    out = np.empty((jones.shape[0], 8), dtype=np.float32)
    for e, (r, c) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
        out[:, 2 * e], out[:, 2 * e + 1] = jones[:, r, c].real, jones[:, r, c].imag
    return out


def random_chirp(n, seed=3):
    """the random-phase response of test_gpu_parity._fb_block: unit modulus, bin 0 zeroed"""
    rng = np.random.default_rng(seed)
    k = np.exp(1j * rng.uniform(-np.pi, np.pi, n)).astype(np.complex64)
    k[0] = 0
    return k


def matrix_response(n, seed=11):
    """one independent Jones matrix per bin times a random-phase chirp with bin 0 zeroed: float32 [n][8]"""
    j = jones_matrices(n, seed) * random_chirp(n, seed + 1).astype(np.complex128)[:, None, None]
    return pack8(j)


def diagonal_response(k):
    """diag(k, k) of a scalar response k (complex64 [n]): f11 = f22 = k, f12 = f21 = 0"""
    m = np.zeros((k.size, 8), dtype=np.float32)
    m[:, 0] = m[:, 4] = k.real
    m[:, 1] = m[:, 5] = k.imag
    return m


def make_plan(o, C, M, nfilt, real):
    N = C * M
    nfilt_pos, nfilt_neg = nfilt
    plan = o.FilterbankPlan(C, 1, C, M, N, nfilt_pos, nfilt_neg, nfilt_pos + nfilt_neg, 2 * N if real else N,
                            (2 if real else 1) * (nfilt_pos + nfilt_neg) * C, 0, M - nfilt_pos - nfilt_neg, float(N) * M, real)
    plan.nsamp_step = plan.nsamp_fft - plan.nsamp_overlap
    return plan


def host_block(o, C, M, nfilt, npart, real=True, seed=3):
    """8-bit dual-polarisation block of one input channel: (plan, obs, raw int8, unpacked float32 [1][2][ndat * ndim])"""
    plan = make_plan(o, C, M, nfilt, real)
    obs = o.Observation(nchan=1, npol=2, ndim=1 if real else 2)
    ndat = npart * plan.nsamp_step + plan.nsamp_overlap
    rng = np.random.default_rng(seed)
    raw = np.clip(np.rint(rng.standard_normal(ndat * 2 * obs.ndim) * 30.0), -128, 127).astype(np.int8)
    return plan, obs, raw, o.unpack_8bit(raw, obs)


def device_block(o, gpu, torch, C, M, nfilt, npart, real=True, use_raw=True, max_parts=1, seed=3, **setup):
    """The engine (no response set yet beyond what `setup` names), the device input and what the restatement needs."""
    dspsr_amd, ctx = gpu
    b = types.SimpleNamespace()
    b.plan, b.obs, raw, b.unpacked = host_block(o, C, M, nfilt, npart, real, seed)
    b.C, b.M, b.npart, b.real = C, M, npart, real
    b.eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, nfilt[0], nfilt[1], 1, 2, real, max_parts=max_parts, **setup)
    assert (b.eng.nsamp_fft, b.eng.nsamp_overlap, b.eng.nsamp_step, b.eng.nkeep) == \
        (b.plan.nsamp_fft, b.plan.nsamp_overlap, b.plan.nsamp_step, b.plan.nkeep)
    b.scale = float(o.S8)
    b.layout = dspsr_amd.RAW_GENERIC
    if use_raw:
        b.raw, b.inp, b.in_step = torch.from_numpy(raw).cuda(), None, 0
    else:
        b.raw, b.inp, b.in_step = None, torch.from_numpy(b.unpacked).cuda(), b.plan.nsamp_step * b.obs.ndim
    return b


def run_complex(b, torch):
    """the complex filterbank output of the block's engine as it stands: complex64 [C][2][npart * nkeep]"""
    out = torch.zeros((b.C, 2, 2 * b.npart * b.plan.nkeep), dtype=torch.float32, device="cuda")
    if b.raw is not None:
        b.eng.perform_raw(b.raw, b.layout, b.scale, out, b.npart)
    else:
        b.eng.perform(b.inp, out, b.npart, b.in_step, 2 * b.plan.nkeep)
    b.eng.finish()
    got = out.cpu().numpy().view(np.complex64)
    assert np.isfinite(got).all()
    return got
