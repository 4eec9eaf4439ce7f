"""Host side of the matrix response (`dspsr -pac`): the numpy restatement of tests/matrix_cases.py against itself and against the
oracle, and dspsr_amd/polcal.py -- element order, product with the chirp, and the sky frequency of every response bin."""
import math

import numpy as np
import pytest

import matrix_cases as mc


@pytest.mark.parametrize("C,M,nfilt,real", [(16, 256, (20, 21), True), (1024, 16, (1, 2), True), (4, 4096, (422, 422), True),
                                            (32, 128, (9, 10), False)])
def test_float32_restatement_meets_the_filterbank_bound(oracle, C, M, nfilt, real):
    """rms(err) / rms(out) <= 2e-6 sqrt(log2(2 C M)), max <= 8x that: the reference's own float32 arithmetic sits about 50x
    inside (relative rms 0.9e-7 ... 1.4e-7 against tol ~ 7.5e-6)"""
    plan, _, _, unpacked = mc.host_block(oracle, C, M, nfilt, 2, real)
    m8 = mc.matrix_response(C * M)
    lo = mc.filterbank_matrix(unpacked, plan, m8, 2, dtype=np.float32)
    hi = mc.filterbank_matrix(unpacked, plan, m8, 2, dtype=np.float64)
    assert lo.dtype == np.complex64 and hi.dtype == np.complex128
    mc.assert_fb_bound(lo, hi, C, M)


@pytest.mark.parametrize("real", [True, False])
def test_diagonal_matrix_is_the_scalar_response(oracle, real):
    C, M, nfilt = 16, 256, (20, 21)
    plan, _, _, unpacked = mc.host_block(oracle, C, M, nfilt, 2, real)
    k = mc.random_chirp(C * M)
    want = oracle.filterbank(unpacked, plan, k, npart=2, dtype=np.float64)
    got = mc.filterbank_matrix(unpacked, plan, mc.diagonal_response(k), 2, dtype=np.float64)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_condition_number_of_the_generated_matrices():
    j = mc.jones_matrices(4096)
    s = np.linalg.svd(j, compute_uv=False)
    assert (s[:, 0] / s[:, 1]).max() <= 4.0 + 1e-9 and s.min() >= 0.5 - 1e-9 and s.max() <= 2.0 + 1e-9


def _obs(oracle, real, bw=-16.0, freq=1382.0, dm=0.0):
    return oracle.Observation(centre_frequency=freq, bandwidth=bw, nchan=1, npol=2, ndim=1 if real else 2, dispersion_measure=dm)


@pytest.mark.parametrize("real", [True, False])
def test_jones_response_element_order(oracle, real):
    from dspsr_amd import polcal
    j = np.array([[[1 + 2j, 3 + 4j], [5 + 6j, 7 + 8j]]])                     # f11 f12 / f21 f22
    r = polcal.jones_response(np.array([1400.0]), j, _obs(oracle, real), 8, 4)
    assert r.shape == (32, 8) and r.dtype == np.float32
    assert np.array_equal(r, np.tile(np.array([1, 2, 5, 6, 7, 8, 3, 4], np.float32), (32, 1)))     # f11, f21, f22, f12


def test_jones_response_takes_the_nearest_calibrator_channel(oracle):
    from dspsr_amd import polcal
    obs = _obs(oracle, True, bw=-16.0)
    nchan, M = 4, 8
    centre, offset = polcal.response_bin_frequencies(obs, nchan, M)
    # one calibrator channel per output channel, in scrambled order, each a multiple of the unit matrix
    cf = np.array([oracle.observation_channel_frequency(obs, c, nchan) for c in range(nchan)])
    order = np.array([2, 0, 3, 1])
    jones = np.eye(2)[None] * (1.0 + order)[:, None, None]
    r = polcal.jones_response(cf[order], jones, obs, nchan, M)
    sky = centre + offset
    # (the first bin of a channel lies on the edge between two calibrator channels: the documented tie goes to the lower frequency)
    want = np.array([1.0 + min(np.flatnonzero(np.abs(cf - f) <= np.abs(cf - f).min() + 1e-9), key=lambda c: cf[c]) for f in sky],
                    np.float32)
    assert len(set(want.tolist())) == nchan
    assert np.array_equal(r[:, 0], want) and np.array_equal(r[:, 4], want)
    assert not r[:, [1, 2, 3, 5, 6, 7]].any()


def test_response_product(oracle):
    from dspsr_amd import polcal
    n = 4096
    m8 = mc.pack8(mc.jones_matrices(n, seed=5))
    k = mc.random_chirp(n, seed=6)
    got = polcal.response_product(m8, k)
    assert got.dtype == np.float32 and got.shape == (n, 8)
    j = (m8[:, 0::2].astype(np.float64) + 1j * m8[:, 1::2].astype(np.float64)) * k.astype(np.complex128)[:, None]
    assert np.abs(got[:, 0::2] - j.real).max() <= 4e-7 * 2.0 and np.abs(got[:, 1::2] - j.imag).max() <= 4e-7 * 2.0
    # float32 by the formula of Response.C:429-441, element by element
    fr, fi = k.real.astype(np.float32), k.imag.astype(np.float32)
    for e in range(4):
        dr, di = m8[:, 2 * e], m8[:, 2 * e + 1]
        assert np.array_equal(got[:, 2 * e], fr * dr - fi * di) and np.array_equal(got[:, 2 * e + 1], fi * dr + fr * di)
    assert not got[0].any(), "bin 0 of the chirp is zero"


@pytest.mark.parametrize("real", [True, False], ids=["real", "complex"])
def test_bin_frequencies_agree_with_the_chirp(oracle, real):
    """The phasors recomputed in float64 from the returned (centre, offset) by SURVEY Appendix A.1 match the kernel
    dspsr_amd_dedispersion_build returns, bin 0 excepted, to 2e-3: float32 phases below 1e3 rad are quantised to ~1e-4 rad."""
    import dspsr_amd
    from dspsr_amd import polcal
    freq, bw, dm, nchan = 1382.0, -16.0, 30.0, 16
    obs = _obs(oracle, real, bw, freq, dm)
    resp = dspsr_amd.Dedispersion(freq, bw, dm, ndim=1 if real else 2).match(nchan)
    M = resp.ndat
    centre, offset = polcal.response_bin_frequencies(obs, nchan, M)
    assert centre.shape == offset.shape == (nchan * M,)
    sign = bw / abs(bw)
    disp = 1e6 * dm / 2.41e-4
    phase = -sign * 2 * math.pi * disp / (centre * centre) * offset * offset / (centre + offset)
    assert np.abs(phase).max() < 1e3, "the test's geometry must keep the float32 phases fine"
    assert np.abs(phase).max() > 10.0, "... and the chirp must wind: a flat response would match any order"
    want = np.exp(1j * phase)
    d = np.abs(resp.kernel.astype(np.complex128) - want)
    # the zeroed bins: bin 0 as built (Dedispersion.C:323) -- for complex input moved to N / 2 by the half swap -- and bin 0 of
    # the matched response (Dedispersion.C:278)
    zeroed = [0] if real else [0, nchan * M // 2]
    assert not resp.kernel[zeroed].any()
    d[zeroed] = 0
    assert d.max() <= 2e-3, d.max()


@pytest.mark.parametrize("real,bw", [(True, -16.0), (False, 16.0)], ids=["real-lower-sideband", "complex"])
def test_frequency_dependent_zap(oracle, real, bw):
    """A scalar kernel that is 0 where the returned frequency lies in a band, else 1, through oracle.filterbank in float64: zapping
    the band of the channel a tone falls in removes the tone, zapping any other channel's band leaves it alone."""
    from dspsr_amd import polcal
    freq, nchan, M = 1382.0, 8, 32
    obs = _obs(oracle, real, bw, freq)
    plan = mc.make_plan(oracle, nchan, M, (0, 0), real)
    ndim = 1 if real else 2
    n = plan.nsamp_fft
    # a pure tone exactly on a bin of the part's spectrum (so that it does not leak), inside one output channel
    kbin = 3 * M + M // 2 + 3
    t = np.arange(n)
    if real:
        x = np.cos(2 * np.pi * kbin * t / n)
    else:
        x = np.exp(2j * np.pi * kbin * t / n).view(np.float64)
    unpacked = np.broadcast_to(x.astype(np.float64), (1, 2, n * ndim)).copy()
    plain = oracle.filterbank(unpacked, plan, None, npart=1, dtype=np.float64)
    power = (np.abs(plain[:, 0]) ** 2).sum(axis=1)
    chan = int(np.argmax(power))
    assert power[chan] > 0.999 * power.sum(), "the tone must sit in one output channel"
    centre, offset = polcal.response_bin_frequencies(obs, nchan, M)
    sky = centre + offset
    half = 0.5 * abs(bw) / nchan
    oobs = oracle.filterbank_output_observation(obs, plan)            # (complex input: the output channels are in swapped order)
    for c in range(nchan):
        fc = oracle.observation_channel_frequency(oobs, c, nchan, swap=oobs.swap)
        # the closed band [f1, f2]: the channel's freq_res bins and, inside the band, the edge bin it shares with a neighbour
        kernel = np.where((sky >= fc - half - 1e-9) & (sky <= fc + half + 1e-9), 0.0, 1.0).astype(np.complex64)
        assert M <= (kernel == 0).sum() <= M + 1, "a channel's band holds freq_res bins and at most one shared edge"
        out = oracle.filterbank(unpacked, plan, kernel, npart=1, dtype=np.float64)
        p = (np.abs(out[:, 0]) ** 2).sum()
        if c == chan:
            assert p < 1e-6 * power.sum(), (c, p / power.sum())
        else:
            assert abs(p - power.sum()) <= 1e-6 * power.sum(), (c, p / power.sum())


def test_refusals_of_the_host_functions(oracle):
    import dspsr_amd
    from dspsr_amd import polcal
    with pytest.raises(dspsr_amd.DspsrAmdError):
        polcal.response_bin_frequencies(oracle.Observation(nchan=2, ndim=2), 8, 4)
    with pytest.raises(dspsr_amd.DspsrAmdError):
        polcal.jones_response(np.array([1.0, 2.0]), np.eye(2)[None], _obs(oracle, True), 8, 4)
    with pytest.raises(dspsr_amd.DspsrAmdError):
        polcal.response_product(np.zeros((8, 8), np.float32), np.zeros(7, np.complex64))


def test_load_calibrator(tmp_path, oracle):
    from dspsr_amd import polcal
    p = tmp_path / "cal.npz"
    np.savez(p, freq=np.array([1400.0, 1380.0]), jones=np.stack([np.eye(2), 2j * np.eye(2)]))
    f, j = polcal.load_calibrator(str(p))
    assert f.tolist() == [1400.0, 1380.0] and j.shape == (2, 2, 2) and j[1, 0, 0] == 2j
