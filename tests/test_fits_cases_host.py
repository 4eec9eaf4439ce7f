"""What tests/test_gpu_fits.py and tests/test_gpu_fits_pipeline.py rely on, checked without a GPU: the restatement of dsp::FITSDigitizer
(tests/fits_cases.py) gives hand-computed answers, its cases reach their edges, its noise case is fair, and pipeline.LoadToFITS plans
and refuses as LoadToFITS.C does -- the constructors plan before they open a device."""
import dataclasses
import math

import numpy as np
import pytest

import fits_cases as fc

f32, f64 = np.float32, np.float64


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def test_two_channels_four_samples_two_bits_by_hand():
    """chan 0 = (1, 3, 1, 3): sum 8, squares 20, offset 2, scale sqrt(5 - 4) = 1; chan 1 = (0, 0, 8, 8): 16, 128, offset 4, scale
    sqrt(32 - 16) = 4.  Levels int(tmp + 1.5 + 0.5): tmp -1 -> 1, +1 -> 3; the TPF samples (t, chan) = 1 1 | 3 1 | 1 3 | 3 3, four to a
    byte, first sample in the top bits: 0b01011101, 0b01111111."""
    x = np.array([[[1, 3, 1, 3]], [[0, 0, 8, 8]]], f32)
    d = fc.FITSDigitizer(2, 1, 2, 4)
    data, scl, offs = d.pack(x)
    assert d.offset.tolist() == [2.0, 4.0] and d.scale.tolist() == [1.0, 4.0]
    assert data.tolist() == [0b01011101, 0b01111111]
    assert scl.tolist() == [1.0, 4.0] and offs.tolist() == [2.0, 4.0] and scl.dtype == offs.dtype == f32       # digi_scale 1 at 2 bits
    assert fc.unpack_levels(data, 2).tolist() == [1, 1, 3, 1, 1, 3, 3, 3]
    # 8 bits: digi_scale 127.5 / 8; tmp = -1 -> int(-15.9375 + 127.5 + 0.5) = 112, +1 -> 143; DAT_SCL = scale / 15.9375
    data, scl, offs = fc.FITSDigitizer(2, 1, 8, 4).pack(x)
    assert data.tolist() == [112, 112, 143, 112, 112, 143, 143, 143]
    assert scl.tolist() == [f32(1.0 / 15.9375), f32(4.0 / 15.9375)]
    # 4 bits and 1 bit: two and eight samples to a byte
    assert fc.FITSDigitizer(2, 1, 4, 4).pack(x)[0].tolist() == [0x77, 0x87, 0x78, 0x88]       # int(-+0.9375 + 7.5 + 0.5) = 7, 8
    assert fc.FITSDigitizer(2, 1, 1, 4).pack(x)[0].tolist() == [0b00100111]                   # int(-+1 + 0.5 + 0.5) = 0, 1
    assert [fc.digi_scales(b)[1:] for b in (1, 2, 4, 8)] == [(1.0, 0, 1), (1.0, 0, 3), (0.9375, 0, 15), (15.9375, 0, 255)]
    with pytest.raises(ValueError, match="nbit=16 not understood"):
        fc.digi_scales(16)


def test_a_constant_row_and_a_huge_value_take_the_clip_paths():
    """constant row (nsblk a power of two: mean and mean square exact): scale 0, m_scale = float(1/0) = inf, tmp = 0 * inf = NaN,
    the conversion gives INT_MIN, the clip digi_min; a row holding one 3e38: its float square is inf, scale inf, m_scale 0, every
    level int(digi_mean + 0.5); a row holding one 1e15 among 63 values of 37: the outlier lies sqrt(63) = 7.9 sigma out and takes
    digi_max below 8 bits (at 8: int(7.937 * 15.9375 + 128) = 254)"""
    for nbit in (1, 2, 4, 8):
        x = np.full((8, 1, 64), 37.0, f32)
        x[1, 0] = np.arange(64) % 5
        x[2, 0, 7] = 3e38
        x[3, 0, 9] = 1e15
        d = fc.FITSDigitizer(8, 1, nbit, 64)
        data, scl, offs = d.pack(x)
        lev = fc.unpack_levels(data, nbit).reshape(64, 8)
        assert d.scale[0] == 0.0 and scl[0] == 0.0 and offs[0] == 37.0 and (lev[:, 0] == 0).all()
        assert math.isinf(d.scale[2]) and math.isinf(scl[2]) and (lev[:, 2] == int(d.digi_mean + 0.5)).all()
        assert lev[9, 3] == (d.digi_max if nbit < 8 else 254) and (np.delete(lev[:, 3], 9) == int(d.digi_mean - 0.126 * d.digi_scale + 0.5)).all()
        assert lev[:, 1].min() < lev[:, 1].max()                                               # an ordinary row beside them
        assert np.array_equal(fc.fast_pack(fc.FITSDigitizer(8, 1, nbit, 64), x)[0], data)
    assert fc.to_int(f64("nan")) == fc.to_int(3e9) == fc.to_int(-3e9) == fc.INT_MIN and fc.to_int(-2147483648.5) == -2 ** 31
    assert fc.to_int(-0.9) == 0 and fc.to_int(2.9) == 2 and fc.to_int(-1.5) == -1               # truncation


def test_flip_and_swap_maps():
    assert fc.channel_map(8, False, False) == list(range(8))
    assert fc.channel_map(8, True, False) == [7, 6, 5, 4, 3, 2, 1, 0]
    assert fc.channel_map(8, False, True) == [4, 5, 6, 7, 0, 1, 2, 3]
    assert fc.channel_map(8, True, True) == [3, 2, 1, 0, 7, 6, 5, 4]
    # output channel k carries input channel map[k]: its levels and its scales
    rng = np.random.default_rng(3)
    x = fc.exact_block(rng, 8, 2, 16)
    plain = fc.FITSDigitizer(8, 2, 8, 16)
    data, scl, offs = plain.pack(x)
    for flip, swap in ((True, False), (False, True), (True, True)):
        m = fc.channel_map(8, flip, swap)
        d2, s2, o2 = fc.FITSDigitizer(8, 2, 8, 16, flip_band=flip, swap_band=swap).pack(x)
        assert np.array_equal(d2.reshape(16, 2, 8), data.reshape(16, 2, 8)[:, :, m])
        assert np.array_equal(s2.reshape(2, 8), scl.reshape(2, 8)[:, m]) and np.array_equal(o2.reshape(2, 8), offs.reshape(2, 8)[:, m])


# ---- the exact generator ------------------------------------------------------------------------------------------------------------
def test_exact_blocks_have_exact_sums_at_the_largest_block():
    rng = np.random.default_rng(1)
    x = fc.exact_block(rng, 6, 2, fc.NSBLK_MAX)
    assert x.dtype == f32 and np.abs(x).max() <= fc.EXACT_MAX and np.array_equal(x, np.rint(x))
    assert np.abs(x).max() == fc.EXACT_MAX                                                      # the clip is reached
    assert fc.NSBLK_MAX * fc.EXACT_MAX ** 2 < 2 ** 53
    for row in x.reshape(-1, fc.NSBLK_MAX):
        xd, sq = row.astype(f64), (row * row).astype(f64)
        for v in (xd, sq):
            assert np.cumsum(v)[-1] == np.cumsum(v[::-1])[-1] == math.fsum(v) == np.sum(v)     # forward, reversed, exact, pairwise
        assert fc.row_sums_sequential(row[:300]) == fc.row_sums_cumsum(row[:300]) == fc.row_sums_pairwise(row[:300])
    with pytest.raises(AssertionError, match="not exact in double"):
        fc.exact_block(rng, 1, 1, 2 ** 31 + 1)


def test_cumsum_is_the_sequential_sum_on_inexact_data():
    rng = np.random.default_rng(5)
    x = fc.noise_block(rng, 3, 1, 1000)
    for row in x.reshape(-1, 1000):
        assert fc.row_sums_sequential(row) == fc.row_sums_cumsum(row)


def test_fast_pack_is_the_loop():
    rng = np.random.default_rng(7)
    for nbit, npol, flip, swap in ((1, 1, False, True), (2, 4, True, False), (4, 2, True, True), (8, 1, False, False)):
        a = fc.FITSDigitizer(8, npol, nbit, 33, nblock=2, flip_band=flip, swap_band=swap)
        b = fc.FITSDigitizer(8, npol, nbit, 33, nblock=2, flip_band=flip, swap_band=swap, row_sums=fc.row_sums_cumsum)
        for _ in range(4):
            x = fc.noise_block(rng, 8, npol, 33)
            want, got = a.pack(x), fc.fast_pack(b, x)
            for w, g in zip(want, got):
                assert w.dtype == g.dtype and np.array_equal(w.view(np.uint8), g.view(np.uint8))


# ---- the ring -----------------------------------------------------------------------------------------------------------------------
def test_ring_cases_visit_every_regime_and_wrap_twice():
    rng = np.random.default_rng(11)
    for nblock in (1, 2, 3):
        n = fc.ring_calls(nblock)
        d = fc.FITSDigitizer(8, 1, 8, 16, nblock=nblock)
        idx = []
        for _ in range(n):
            d.pack(fc.exact_block(rng, 8, 1, 16))
            idx.append(d.rescale_idx)
        if nblock == 1:
            assert d.regimes == ["single"] * n and idx == [0] * n
            continue
        assert d.regimes == ["filling"] * nblock + ["full"] * (nblock + 3)
        assert idx.count(nblock) >= 3                                                          # filled once, wrapped at least twice
        assert d.rescale_counter == nblock
    # old_idx = rescale_idx + 1: with nblock 2 the row subtracted is the OTHER row, i.e. the newer of the two old blocks, not the one
    # just overwritten -- after three blocks a, b, c the running offset is mean(a, b) + (c - b) / 2, not mean(b, c)
    d = fc.FITSDigitizer(8, 1, 8, 4, nblock=2)
    a, b, c = (np.full((8, 1, 4), v, f32) for v in (2.0, 4.0, 10.0))
    for x in (a, b, c):
        d.pack(x)
    assert d.offset[0] == 3.0 + (10.0 - 4.0) / 2 == 6.0 and d.offset[0] != 7.0
    # constant: the first block's pair stays
    d = fc.FITSDigitizer(8, 1, 8, 16, constant=True)
    first = d.pack(fc.exact_block(rng, 8, 1, 16))
    for _ in range(3):
        nxt = d.pack(fc.exact_block(rng, 8, 1, 16))
        assert np.array_equal(nxt[1], first[1]) and np.array_equal(nxt[2], first[2])
    assert d.regimes == ["single", "constant", "constant", "constant"]


# ---- the noise case is fair -------------------------------------------------------------------------------------------------------
def test_noise_case_is_fair():
    """The restatement with sequential sums and with numpy's pairwise sums -- two legitimate orders -- agrees within the cap that
    tests/test_gpu_fits.py sets for the device: levels at most 1 apart on at most 1e-5 of the samples, scales within a float ulp."""
    nchan, npol, nsblk = fc.NOISE_SHAPE
    for nbit in (2, 8):
        rng = np.random.default_rng(fc.NOISE_SEED)
        x = fc.noise_block(rng, nchan, npol, nsblk)
        a = fc.fast_pack(fc.FITSDigitizer(nchan, npol, nbit, nsblk, row_sums=fc.row_sums_cumsum), x)
        b = fc.fast_pack(fc.FITSDigitizer(nchan, npol, nbit, nsblk, row_sums=fc.row_sums_pairwise), x)
        d = np.abs(fc.unpack_levels(a[0], nbit) - fc.unpack_levels(b[0], nbit))
        assert d.max() <= 1 and (d != 0).sum() <= fc.LEVEL_FRACTION * d.size
        for u, v in zip(a[1:], b[1:]):
            assert (np.abs(u.view(np.int32) - v.view(np.int32)) <= 1).all()
        lev = fc.unpack_levels(a[0], 8) if nbit == 8 else None
        if lev is not None:
            assert ((lev > 0) & (lev < 255)).mean() >= 0.99


# ---- LoadToFITS: plan arithmetic and refusals ---------------------------------------------------------------------------------------
def _pipeline():
    from dspsr_amd import pipeline
    return pipeline


REAL = dict(centre_frequency=1400.0, bandwidth=-16.0, nchan=1, npol=2, ndim=1, tsamp_us=1.0 / 32.0, machine="DADA")
CHANNELISED = dict(centre_frequency=1400.0, bandwidth=4.0, nchan=4, npol=2, ndim=2, tsamp_us=1.0, machine="DADA")


def test_plan_arithmetic_at_hand_worked_points():
    p = _pipeline()
    real, chans = p.InputInfo(**REAL), p.InputInfo(**CHANNELISED)
    # real input at 32 MHz, -F 16, -t 64e-6: 2048 voltage samples per output sample, factor 0.5: round(0.5 * 2048 / 16) = 64;
    # tsamp = 64 / 0.5 * 16 / 32e6 = 64e-6
    tres, tsamp, nblock = p.fits_plan(p.FitsConfig(nchan=16, tsamp=64e-6), real)
    assert (tres, nblock) == (64, 1) and tsamp == 64 / 0.5 * 16 / real.rate
    # -t 70e-6: 0.5 * 2240 / 16 = 70 -> 70; -t 71e-6: 71 -> 71; -t 64.5e-6: 64.5 -> 65 (halves go up)
    assert p.fits_plan(p.FitsConfig(nchan=16, tsamp=70e-6), real)[0] == 70
    assert p.fits_plan(p.FitsConfig(nchan=16, tsamp=64.5e-6), real)[0] == p._c_round(0.5 * (64.5e-6 * real.rate) / 16)
    assert p._c_round(64.5) == 65 and p._c_round(2.5) == 3 and p._c_round(2.49) == 2
    # no -F, 4 complex channels at 1 MHz each, -t 16e-6: round(1e6 * 16e-6) = 16, tsamp = 16 / 1 * 1 / 1e6
    tres, tsamp, _ = p.fits_plan(p.FitsConfig(nchan=0, tsamp=16e-6), chans)
    assert tres == 16 and tsamp == 16 / 1.0 * 1 / chans.rate
    # the multi-channel quirk with -F: 4 channels in, -F 16 (a 4-channel filterbank on each), -t 64e-6: the reference counts the
    # per-channel rate against all 16 channels: round(1.0 * 64 / 16) = 4, printed tsamp 64e-6 -- the chain delivers 4 * 4 us = 16 us
    tres, tsamp, _ = p.fits_plan(p.FitsConfig(nchan=16, tsamp=64e-6), chans)
    assert tres == 4 and tsamp == 4 / 1.0 * 16 / chans.rate
    lt = p.LoadToFITS(p.FitsConfig(nchan=16, tsamp=64e-6, npol=1), chans, device=None)          # (the host plan alone)
    assert lt.out_rate == chans.rate / 4 / 4 and lt.header_values()["TBIN"] == 16e-6
    # nblock: -I 1 with 64e-6 * 2048 = 0.131072 s blocks: unsigned(7.629 + 0.5) = 8; -I 0.01: max(1, 0) = 1; -c wins over -I
    assert p.fits_plan(p.FitsConfig(nchan=16, rescale_seconds=1.0), real)[2] == 8
    assert p.fits_plan(p.FitsConfig(nchan=16, rescale_seconds=0.01), real)[2] == 1
    assert p.fits_plan(p.FitsConfig(nchan=16, rescale_seconds=0.19), real)[2] == 1 and p.fits_plan(p.FitsConfig(nchan=16, rescale_seconds=0.2), real)[2] == 2
    assert p.fits_plan(p.FitsConfig(nchan=16, rescale_seconds=1.0, rescale_constant=True), real)[2] == 1
    assert p.fits_plan(p.FitsConfig(nchan=16), real)[2] == 1                                    # -I unset (-1)
    # the defaults of LoadToFITS::Config
    c = p.FitsConfig()
    assert (c.nchan, c.freq_res, c.dispersion_measure, c.dedisperse, c.coherent_dedisp, c.rescale_seconds, c.rescale_constant,
            c.nbit, c.npol, c.nsblk, c.tsamp) == (0, 0, 0.0, False, False, -1, False, 2, 4, 2048, 64e-6)


def test_plan_geometry_and_header_values():
    p = _pipeline()
    real = p.InputInfo(**REAL, start_seconds=0.25, mjd_day=55299, mjd_sec=100.0, source="J0437-4715")
    lt = p.LoadToFITS(p.FitsConfig(nchan=16, convolve=True, freq_res=4, dispersion_measure=10.0, coherent_dedisp=True, npol=2, nbit=4,
                                   nsblk=128), real, device=None)
    assert lt.sd.delays is None
    r = lt.front.response
    assert r.ndat == 4 * r.minimum_ndat                                                         # -x times the minimum (LoadToFITS.C:272)
    hv = lt.header_values()
    assert hv == dict(NSBLK=128, TBIN=1.0 / lt.out_rate, NBITS=4, ZERO_OFF=7.5, NCHAN=16, NPOL=2, POL_TYPE="AABB", OBSFREQ=1400.0, OBSBW=-16.0,
                      CHAN_BW=-1.0, STT_IMJD=55299, STT_SECONDS=100.0 + lt.out_start, SRC_NAME="J0437-4715")
    assert lt.out_rate == 32e6 / 2 / 16 / 64 and lt.out_start == 0.25 + r.impulse_pos / (32e6 / 32)
    assert lt.block_bytes_out == 128 * 2 * 16 // 2
    # no response: -F 16 alone runs the filterbank at freq_res 1, -x 8 at 8; incoherent -D leaves the filterbank without a kernel
    lt = p.LoadToFITS(p.FitsConfig(nchan=16, npol=1), real, device=None)
    assert (lt.front.response.ndat, lt.front.response.kernel) == (1, None)
    lt = p.LoadToFITS(p.FitsConfig(nchan=16, freq_res=8, dispersion_measure=10.0, npol=1), real, device=None)
    assert (lt.front.response.ndat, lt.front.response.kernel) == (8, None)
    # -K: delays of the 16 output channels at the scrunched rate; the start moves by the largest
    lt = p.LoadToFITS(p.FitsConfig(nchan=16, freq_res=8, dispersion_measure=300.0, npol=1, dedisperse=True), real, device=None)
    delays = lt.sd.delays
    assert len(delays) == 16 and lt.sd.head == int(delays.max() - delays.min()) > 0
    assert lt.out_start == lt.front.out_start + int(delays.max()) / lt.out_rate


def test_plan_time_refusals_by_name():
    p = _pipeline()
    real, chans = p.InputInfo(**REAL), p.InputInfo(**CHANNELISED)
    ok = dict(nchan=16, npol=1)

    def refused(match, info=real, **kw):
        with pytest.raises(p.DspsrAmdError, match=match):
            p.LoadToFITS(p.FitsConfig(**{**ok, **kw}), info, device=10 ** 6)        # (a device that does not exist: never reached)

    detected = dataclasses.replace(real)
    detected.detected = True
    refused("detected input", info=detected)
    refused("-do_dedisp without -F N:D", dispersion_measure=10.0, coherent_dedisp=True)
    refused("-do_dedisp without -F N:D", info=chans, nchan=0, dispersion_measure=10.0, coherent_dedisp=True)
    refused("two-bit input", info=dataclasses.replace(real, nbit=2))
    refused("must specify filterbank scheme if single channel data", nchan=0)
    refused("heap order of INSTRUMENT MKBFRo", info=dataclasses.replace(chans, machine="MKBFRo"), nchan=0)
    refused("CASPSR byte order", info=dataclasses.replace(chans, machine="CASPSR"), nchan=0)
    refused("-L ", integration_length=10.0)
    refused("invalid polarization specified", npol=3)
    refused("nbit=16 not understood", nbit=16)
    refused("nbit=3 not understood", nbit=3)
    refused("not a multiple of 8 samples per byte", info=chans, nchan=12, nbit=1)
    refused("scrunch factor not set", tsamp=1e-7)
    refused("-F 1 ", nchan=1)
    refused("not a multiple of input nchan", info=chans, nchan=6)
    refused("need two input polarisations", info=dataclasses.replace(real, npol=1), npol=2)
