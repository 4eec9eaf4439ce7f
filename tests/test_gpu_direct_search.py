"""Search mode on already channelised 8-bit voltages, `digifil file.dada` with no -F (LoadToFil.C:233-362): the stand-alone unpacker
(dspsr_amd.unpack_fpt), the one-pass front end (dspsr_amd.detect_raw = unpack -> Detection -> TScrunch) and pipeline.LoadToFilDirect
against the unfused chain of existing calls (bit for bit) and against the oracle (derived bounds)."""
import numpy as np
import pytest

from device_buffers import SENTINEL, OutputLayout, sentinel_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 20100413
EPS = 4.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


def noise(rng, n):
    """Gaussian int8 noise, sigma = 24 LSB (as synth.py)"""
    return np.clip(np.rint(rng.normal(0.0, 24.0, n)), -128, 127).astype(np.int8)


def odd_device_bytes(raw, skew=1):
    """the block on the device, `skew` bytes past a 256-byte boundary"""
    buf = torch.empty(raw.size + 512, dtype=torch.int8, device="cuda")
    lead = (-buf.data_ptr()) % 256 + skew
    view = buf[lead:lead + raw.size]
    view.copy_(torch.from_numpy(raw))
    assert view.data_ptr() % 256 == skew
    return view


def untouched(buf, lay, rows_written):
    """every int32 of the sentinel buffer outside the first `rows_written` floats of each row still holds the sentinel"""
    bits = buf.cpu().numpy().copy()
    for c in range(lay.nchan):
        for p in range(lay.nplanes):
            r0 = lay.first + c * lay.chan_stride + p * lay.pol_stride
            bits[r0:r0 + rows_written] = SENTINEL
    return bool((bits == SENTINEL).all())


STATES = {"Intensity": 1, "PPQQ": 2, "Coherence": 4}


def state_id(dspsr_amd, name):
    return {"Intensity": dspsr_amd.INTENSITY, "PPQQ": dspsr_amd.PPQQ, "Coherence": dspsr_amd.COHERENCE}[name]


# ---- 1. the unpacker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan,npol,ndim", [(1, 2, 2), (8, 2, 2), (81, 2, 2), (64, 1, 2), (1000, 2, 2), (4096, 2, 2), (1024, 4, 1), (3, 1, 1)])
def test_unpack_fpt_bit_exact(oracle, gpu, nchan, npol, ndim):
    """unpack_fpt == oracle.unpack_8bit bit for bit; the raw pointer at an odd byte address (and at an aligned one: the word loads),
    rows cut from a sentinel buffer with padded strides that no store may leave."""
    dspsr_amd, ctx = gpu
    rng = np.random.default_rng(SEED)
    obs = oracle.Observation(nchan=nchan, npol=npol, ndim=ndim)
    for ndat in (1, 63, 4097):
        raw = noise(rng, ndat * nchan * npol * ndim)
        k = min(4, raw.size)
        raw[:k] = np.array((-128, 127, 0, -1), np.int8)[:k]                 # the ends of the range
        want = oracle.unpack_8bit(raw, obs)
        for skew, offset, pad in ((1, 1, 3), (0, 2, 1), (3, 0, 0)):
            lay = OutputLayout(nchan, npol, ndat * ndim, offset, pad)
            buf, rows = sentinel_rows(lay)
            dspsr_amd.unpack_fpt(ctx, odd_device_bytes(raw, skew), rows, nchan, npol, ndim, float(oracle.S8))
            assert np.array_equal(rows.cpu().numpy(), want), (ndat, skew)
            assert untouched(buf, lay, ndat * ndim), (ndat, skew)


# ---- 2. fused == unfused --------------------------------------------------------------------------------------------------------
def unfused(dspsr_amd, ctx, d_raw, nchan, npol, state, sf, scale):
    """unpack_fpt -> detect_square_law / detect_polarimetry(COHERENCE, ndim 1) -> tscrunch_fpt of a whole stream in one call"""
    ndat = d_raw.numel() // (nchan * npol * 2)
    volt = torch.empty((nchan, npol, 2 * ndat), dtype=torch.float32, device="cuda")
    dspsr_amd.unpack_fpt(ctx, d_raw, volt, nchan, npol, 2, scale)
    det = torch.empty((nchan, STATES[state], ndat), dtype=torch.float32, device="cuda")
    eng = dspsr_amd.DetectionEngine(ctx)
    if state == "Coherence":
        eng.polarimetry(1, volt, det, dspsr_amd.COHERENCE)
    else:
        eng.square_law(volt, det, intensity=state == "Intensity")
    out = torch.empty((nchan, STATES[state], ndat // sf + 1), dtype=torch.float32, device="cuda")
    carry = torch.zeros((nchan, STATES[state]), dtype=torch.float32, device="cuda")
    nout, _ = dspsr_amd.tscrunch_fpt(ctx, det, out, sf, carry, 0)
    assert nout == ndat // sf
    return det, out[:, :, :nout].cpu().numpy()


def fused_stream(dspsr_amd, ctx, raw, nchan, npol, state, sf, scale, calls, skew=0):
    """detect_raw over the stream cut into `calls`; checks nout and carry_count of every call, and that nothing outside the nout
    floats of a row is written"""
    npo = STATES[state]
    per = nchan * npol * 2
    carry = torch.zeros((nchan, npo), dtype=torch.float32, device="cuda")
    cc, pos, got = 0, 0, []
    for k, n in enumerate(calls):
        want_nout = (pos + n) // sf - pos // sf
        lay = OutputLayout(nchan, npo, want_nout + 1, (1, 2, 0, 3)[k % 4], (1, 0, 3)[k % 3])
        buf, rows = sentinel_rows(lay)
        blk = odd_device_bytes(raw[pos * per:(pos + n) * per], skew)
        nout, cc = dspsr_amd.detect_raw(ctx, blk, rows, carry, cc, nchan, npol, sf, state_id(dspsr_amd, state), scale, ndat=n)
        pos += n
        assert nout == want_nout and cc == pos % sf, (k, n, nout, cc)
        assert untouched(buf, lay, nout), (k, n)
        got.append(rows[:, :, :nout].cpu().numpy())
    return np.concatenate(got, axis=2)


CALLS_A = (700, 5, 0, 1400, 1, 300, 19)
CALLS_B = (1, 1023, 1, 399, 1001)
assert sum(CALLS_A) == sum(CALLS_B) == 2425


@pytest.mark.parametrize("nchan", [1, 8, 81, 64, 1000, 4096])
@pytest.mark.parametrize("npol", [1, 2])
def test_detect_raw_equals_the_unfused_chain(oracle, gpu, nchan, npol):
    """Intensity, PPQQ, Coherence x tscrunch 1 ... 1024, a stream of calls of unequal lengths (shorter than the factor, empty):
    the same bits as the three existing calls on the unpacked rows, for either way of cutting the stream; and the oracle's
    numbers within the bounds that one rounding against two of x*x + y*y allows."""
    dspsr_amd, ctx = gpu
    rng = np.random.default_rng(SEED + nchan + npol)
    ndat = sum(CALLS_A)
    raw = noise(rng, ndat * nchan * npol * 2)
    scale = float(oracle.S8)
    d_raw = torch.from_numpy(raw).cuda()
    obs = oracle.Observation(nchan=nchan, npol=npol, ndim=2)
    cplx = oracle.unpack_8bit(raw, obs).view(np.complex64)
    for state in (("Intensity",) if npol == 1 else ("Intensity", "PPQQ", "Coherence")):
        if state == "Coherence":
            odet = np.ascontiguousarray(oracle.detect_layout(oracle.detect_products(cplx, "Coherence"), 1))
        else:
            odet = oracle.square_law(cplx, state)
        for sf in (1, 2, 3, 16, 25, 1024):
            _, want = unfused(dspsr_amd, ctx, d_raw, nchan, npol, state, sf, scale)
            a = fused_stream(dspsr_amd, ctx, raw, nchan, npol, state, sf, scale, CALLS_A, skew=0)
            assert a.shape == want.shape and np.array_equal(a, want), (state, sf, "A")
            b = fused_stream(dspsr_amd, ctx, raw, nchan, npol, state, sf, scale, CALLS_B, skew=(sf % 4))
            assert np.array_equal(b, want), (state, sf, "B")
            # ---- 3. against the oracle
            ow = oracle.tscrunch_fpt(odet, sf).astype(np.float64)
            g = a.astype(np.float64)
            npos = 1 if state == "Intensity" else 2
            err = np.abs(g[:, :npos] - ow[:, :npos])
            print("%s nchan %d npol %d tscrunch %d: max |got - want| / want = %.3g" % (state, nchan, npol, sf, float((err / ow[:, :npos]).max())))
            assert (err <= EPS * ow[:, :npos]).all(), (state, sf)
            if state == "Coherence":
                lim = EPS * np.sqrt(ow[:, 0] * ow[:, 1])
                for r in (2, 3):
                    e = np.abs(g[:, r] - ow[:, r])
                    print("  product %d: max |got - want| / sqrt(PP QQ) = %.3g" % (r, float((e / np.sqrt(ow[:, 0] * ow[:, 1])).max())))
                    assert (e <= lim).all(), (state, sf, r)


# ---- 4. the carry is read before it is replaced ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [1, 4096])
def test_detect_raw_carry_read_before_it_is_replaced(oracle, gpu, nchan):
    """Many short calls that begin AND end inside an output sample (output 0 reads the carry, the open group replaces it), more
    outputs per row than one workgroup holds at 4096 channels: bit-exact against one long call."""
    dspsr_amd, ctx = gpu
    rng = np.random.default_rng(SEED + 4)
    scale = float(oracle.S8)
    for sf in (3, 5, 7):
        calls = tuple(int(x) for x in rng.integers(1, 4 * sf, 40)) + (274, 822, 1000, 2) + tuple(int(x) for x in rng.integers(1, 3 * sf, 40))
        ndat = sum(calls)
        raw = noise(rng, ndat * nchan * 2 * 2)
        for state in ("Intensity", "Coherence"):
            whole = fused_stream(dspsr_amd, ctx, raw, nchan, 2, state, sf, scale, (ndat,))
            for rep in range(2):
                got = fused_stream(dspsr_amd, ctx, raw, nchan, 2, state, sf, scale, calls)
                assert got.shape == whole.shape and np.array_equal(got, whole), (sf, state, rep)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_direct_search_refusals(oracle, gpu):
    """Every misuse is DSPSR_AMD_EINVAL before any launch: the sentinel buffer keeps its pattern, carry_count and nout are not
    touched, and the next valid call works."""
    import ctypes as C
    dspsr_amd, ctx = gpu
    lib = dspsr_amd.lib
    rng = np.random.default_rng(SEED + 5)
    nchan, npol, ndat, sf = 8, 2, 100, 4
    raw = noise(rng, ndat * nchan * npol * 2)
    d_raw = torch.from_numpy(raw).cuda()
    lay = OutputLayout(nchan, 4, 2 * ndat, 1, 1)
    buf, rows = sentinel_rows(lay)
    carry = torch.full((nchan, 4), 7.0, dtype=torch.float32, device="cuda")
    scale = float(oracle.S8)
    I, P, Co = dspsr_amd.INTENSITY, dspsr_amd.PPQQ, dspsr_amd.COHERENCE
    cs, ps = lay.chan_stride, lay.pol_stride

    def detect(nchan=nchan, npol=npol, state=I, ts=sf, ocs=cs, ops=ps, carry_ptr=carry.data_ptr(), cc=1, with_cc=True, ndat=ndat):
        c, n = C.c_uint32(cc), C.c_uint64(12345)
        rc = lib.dspsr_amd_detect_raw(ctx.handle, d_raw.data_ptr(), scale, nchan, npol, ndat, state, ts, rows.data_ptr(), ocs, ops,
                                      carry_ptr, C.byref(c) if with_cc else None, C.byref(n))
        return rc, c.value, n.value

    bad = [dict(nchan=0), dict(npol=4), dict(npol=3), dict(npol=0), dict(state=dspsr_amd.STOKES), dict(state=17), dict(npol=1, state=P),
           dict(npol=1, state=Co), dict(ts=0), dict(carry_ptr=None), dict(with_cc=False), dict(cc=4), dict(cc=9),
           dict(state=P, ops=(1 + ndat) // sf - 1), dict(state=Co, ocs=3 * ps + (1 + ndat) // sf - 1), dict(state=I, ocs=(1 + ndat) // sf - 1)]
    for kw in bad:
        rc, c, n = detect(**kw)
        assert rc == dspsr_amd._lib.EINVAL, kw
        assert (c, n) == (kw.get("cc", 1), 12345), kw
        assert untouched(buf, lay, 0) and bool((carry == 7.0).all()), kw

    def unpack(nchan=nchan, npol=npol, ndim=2, ocs=cs, ops=ps):
        return lib.dspsr_amd_unpack_fpt(ctx.handle, d_raw.data_ptr(), scale, nchan, npol, ndim, ndat, rows.data_ptr(), ocs, ops)
    for kw in [dict(nchan=0), dict(npol=3), dict(npol=0), dict(npol=8), dict(ndim=0), dict(ndim=4), dict(ops=2 * ndat - 1), dict(ocs=ps + 2 * ndat - 1)]:
        assert unpack(**kw) == dspsr_amd._lib.EINVAL, kw
        assert untouched(buf, lay, 0), kw
    # through the Python mirror: DspsrAmdError with the library's text
    with pytest.raises(dspsr_amd.DspsrAmdError, match="scrunch factor not set"):
        dspsr_amd.detect_raw(ctx, d_raw, rows, carry, 0, nchan, npol, 0, I, scale)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="needs two input polarisations"):
        dspsr_amd.detect_raw(ctx, d_raw, rows, carry, 0, 2 * nchan, 1, sf, P, scale)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="needs carry_dev"):
        dspsr_amd.detect_raw(ctx, d_raw, rows, None, 0, nchan, npol, sf, I, scale)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="npol=3"):
        dspsr_amd.unpack_fpt(ctx, d_raw, rows[:, :3], nchan, 3, 2, scale, ndat=10)
    assert untouched(buf, lay, 0)
    # an empty call is a successful no-op; tscrunch 1 needs no carry
    assert detect(ndat=0, cc=3) == (0, 3, 0) and untouched(buf, lay, 0) and bool((carry == 7.0).all())
    assert lib.dspsr_amd_unpack_fpt(ctx.handle, None, scale, nchan, npol, 2, 0, None, 0, 0) == 0
    # the next valid calls work
    obs = oracle.Observation(nchan=nchan, npol=npol, ndim=2)
    volt = oracle.unpack_8bit(raw, obs)
    dspsr_amd.unpack_fpt(ctx, d_raw, rows[:, :npol], nchan, npol, 2, scale)
    assert np.array_equal(rows[:, :npol].cpu().numpy(), volt)
    out = torch.empty((nchan, 1, ndat), dtype=torch.float32, device="cuda")
    nout, cc = dspsr_amd.detect_raw(ctx, d_raw, out, None, None, nchan, npol, 1, I, scale)
    assert (nout, cc) == (ndat, 0) and np.array_equal(out.cpu().numpy(), oracle.square_law(volt.view(np.complex64), "Intensity"))
    carry.zero_()
    nout, cc = dspsr_amd.detect_raw(ctx, d_raw, out, carry, 0, nchan, npol, sf, I, scale)
    assert (nout, cc) == (ndat // sf, 0)
    assert np.array_equal(out[:, :, :nout].cpu().numpy(), oracle.tscrunch_fpt(oracle.square_law(volt.view(np.complex64), "Intensity"), sf))


# ---- 6. the whole chain ---------------------------------------------------------------------------------------------------------
def levels(b, nbit):
    b = np.asarray(b).reshape(-1)
    if nbit in (8, 16):
        return b.astype(np.int64)
    spb = 8 // nbit
    return ((b[:, None].astype(np.int64) >> (np.arange(spb) * nbit)) & ((1 << nbit) - 1)).reshape(-1)


# nchan, input npol, -d, -b, -f, -t, Rescale, bandwidth sign, -K
CHAIN = [
    (8, 2, 1, 8, 0, 16, "on", -1, False),
    (8, 2, 2, 2, 0, 4, "on", +1, False),
    (8, 2, 4, 1, 0, 3, "constant", -1, False),
    (8, 2, 1, -32, 0, 16, "off", +1, False),
    (8, 2, 2, -32, 0, 1, "off", -1, False),
    (8, 2, 4, -32, 4, 5, "off", -1, False),
    (8, 2, 2, 8, 4, 2, "on", -1, False),
    (8, 2, 4, 8, 4, 1, "constant", +1, False),
    (8, 2, 1, 8, 0, 4, "off", -1, False),
    (8, 1, 1, 8, 0, 8, "on", -1, False),
    (81, 2, 1, 8, 0, 16, "on", +1, False),
    (81, 2, 4, 8, 0, 3, "on", -1, False),
    (81, 2, 2, -32, 0, 1, "off", -1, False),
    (81, 2, 4, -32, 0, 7, "off", +1, False),
    (8, 2, 1, 8, 0, 4, "on", -1, True),
    (8, 2, 4, 2, 0, 4, "constant", +1, True),
    (8, 2, 1, 8, 4, 4, "on", +1, True),
    (8, 2, 2, -32, 0, 3, "off", -1, True),
    (81, 2, 2, 8, 0, 16, "on", +1, True),
    (81, 2, 4, -32, 0, 3, "off", -1, True),
]
BLOCKS = (2000, 300, 100, 1500, 0, 700, 2048, 37)


@pytest.mark.parametrize("nchan,npol_in,npol,nbit,fscr,ts,resc,sign,dedisp", CHAIN)
def test_load_to_fil_direct_against_the_oracle(oracle, gpu, nchan, npol_in, npol, nbit, fscr, ts, resc, sign, dedisp):
    """LoadToFilDirect.process_block over blocks of unequal lengths (with -K: delays of several hundred samples, blocks shorter than the
    total delay + tscrunch) against oracle.DigifilCoherent fed the unpacked complex rows.  Float output without Rescale: the bounds
    of the detector; packed levels: at most 1 level apart in at most 1e-4 of the samples (a cap from the issue, not a measurement:
    rounding alone gives < 1e-6 at 8 bit)."""
    dspsr_amd, _ = gpu
    from dspsr_amd import pipeline
    rng = np.random.default_rng(SEED)
    bw = sign * float(nchan)                                  # 1 MHz channels, tsamp 1 us
    dm = (20.0 if nchan == 8 else 2.0) if dedisp else 0.0
    interval = 256
    info = pipeline.InputInfo(centre_frequency=1400.0, bandwidth=bw, nchan=nchan, npol=npol_in, ndim=2, tsamp_us=1.0, machine="DADA",
                              start_seconds=0.5, mjd_day=55299, mjd_sec=7545.0)
    cfg = pipeline.SearchConfig(nchan=4096, tscrunch=ts, nbit=nbit, rescale_seconds=0.0 if resc == "off" else (interval + 0.5) * ts / 1e6,
                                rescale_constant=resc == "constant", parts_per_block=2048, dispersion_measure=dm, fscrunch=fscr, npol=npol,
                                dedisperse=dedisp)
    lt = pipeline.LoadToFilDirect(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
    obs = oracle.Observation(centre_frequency=1400.0, bandwidth=bw, nchan=nchan, npol=npol_in, ndim=2, tsamp_us=1.0, dispersion_measure=dm)
    delays = oracle.dedispersion_sample_delays(obs, nchan, obs.rate) if dedisp else None
    if dedisp:
        total = int(delays.max() - delays.min())
        assert 200 < total < 2000 and BLOCKS[1] < total + ts and lt.sd_head == total
    assert lt.rescale_interval == (0 if resc == "off" else interval)
    ref = oracle.DigifilCoherent(tscrunch=ts, fscrunch=fscr, nbit=nbit, npol_out=npol, rescale_interval=interval, rescale_constant=resc == "constant",
                                 rescale=resc != "off", flip_band=bw > 0, delays=delays, input_scale=float(ts * (fscr or 1)))
    nchan_out = nchan // fscr if fscr else nchan
    worst, ndiff, nsamp = 0, 0, 0
    for n in BLOCKS:
        raw = noise(rng, n * nchan * npol_in * 2)
        assert lt.block_bytes(n) == raw.size
        got = lt.process_block(torch.from_numpy(raw).cuda(), n).cpu().numpy()
        cplx = oracle.unpack_8bit(raw, obs).view(np.complex64).reshape(nchan, npol_in, n)
        if nbit == -32:
            # the oracle's scrunched rows themselves: sign information for the bounds (the digitiser only divides by input_scale)
            det = ref.detect_scrunch(cplx).astype(np.float64)                     # [nchan_out][npol][nout]
            order = oracle.channel_sort(nchan_out, bw > 0, False)
            want = det[order].transpose(2, 1, 0) / float(ts * (fscr or 1))
            g = got.view(np.float32).reshape(want.shape).astype(np.float64)
            npos = 2 if npol == 4 else npol
            assert (np.abs(g[:, :npos] - want[:, :npos]) <= EPS * want[:, :npos]).all()
            if npol == 4:
                lim = EPS * np.sqrt(want[:, 0] * want[:, 1])
                assert (np.abs(g[:, 2] - want[:, 2]) <= lim).all() and (np.abs(g[:, 3] - want[:, 3]) <= lim).all()
            nsamp += want.size
        else:
            want = ref.process(cplx)
            lg, lw = levels(got, nbit), levels(want, nbit)
            assert lg.shape == lw.shape, (n, lg.shape, lw.shape)
            d = np.abs(lg - lw)
            if d.size:
                worst, ndiff, nsamp = max(worst, int(d.max())), ndiff + int((d != 0).sum()), nsamp + d.size
    assert nsamp > 0 and lt.ndat_out * nchan_out * npol == nsamp
    print("levels: worst %d, %d of %d differ" % (worst, ndiff, nsamp))
    assert worst <= 1 and ndiff <= 1e-4 * nsamp
    hv = lt.header_values()
    out_obs = oracle.Observation(centre_frequency=1400.0, bandwidth=-abs(bw), nchan=nchan_out)
    start = 0.5 + (int(delays.max()) / obs.rate if dedisp else 0.0)               # SampleDelay.C:159
    assert hv == dict(fch1=oracle.observation_channel_frequency(out_obs, 0, nchan_out), foff=-abs(bw) / nchan_out, nchans=nchan_out,
                      nbits=32 if nbit == -32 else nbit, tsamp=ts / obs.rate, tstart_mjd=55299 + (7545.0 + start) / 86400.0, nifs=npol)
    lt.synchronize()
    lt.close()
