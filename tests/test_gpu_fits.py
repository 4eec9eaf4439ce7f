"""dspsr_amd.FITSDigitizer (dspsr_amd/csrc/fits_digitize.hip) against the loop restatement of dsp::FITSDigitizer in tests/fits_cases.py:
bit for bit where the reference's sums are exact in any order, within the stated caps on noise (their fairness: tests/test_fits_cases_host.py)."""
import ctypes as C

import numpy as np
import pytest

import fits_cases as fc
from device_buffers import SENTINEL, device_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 20151124
BYTE_SENTINEL = 0xA5
GUARD = 256


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


class Outputs:
    """The three outputs of `ncall` packs, each cut from a sentinel buffer with guards in front, between and behind"""

    def __init__(self, ncall, nbytes, ncol, skew=0):
        self.ncall, self.nbytes, self.ncol, self.skew = ncall, nbytes, ncol, skew
        self.bstep, self.fstep = nbytes + GUARD + skew, ncol + GUARD // 4 + 1
        self.bytes = torch.full((GUARD + ncall * self.bstep,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        self.scl = torch.full((GUARD + ncall * self.fstep,), SENTINEL, dtype=torch.int32, device="cuda")
        self.offs = torch.full((GUARD + ncall * self.fstep,), SENTINEL, dtype=torch.int32, device="cuda")

    def views(self, k):
        b0, f0 = GUARD + self.skew + k * self.bstep, GUARD // 4 + 1 + k * self.fstep
        return (self.bytes[b0:b0 + self.nbytes], self.scl[f0:f0 + self.ncol].view(torch.float32), self.offs[f0:f0 + self.ncol].view(torch.float32))

    def collect(self):
        """[(bytes, scl bits, offs bits)] of every call; asserts that nothing outside them was written"""
        b, s, o = self.bytes.cpu().numpy().copy(), self.scl.cpu().numpy().copy(), self.offs.cpu().numpy().copy()
        got = []
        for k in range(self.ncall):
            b0, f0 = GUARD + self.skew + k * self.bstep, GUARD // 4 + 1 + k * self.fstep
            got.append((b[b0:b0 + self.nbytes].copy(), s[f0:f0 + self.ncol].copy(), o[f0:f0 + self.ncol].copy()))
            b[b0:b0 + self.nbytes] = BYTE_SENTINEL
            s[f0:f0 + self.ncol] = SENTINEL
            o[f0:f0 + self.ncol] = SENTINEL
        assert (b == BYTE_SENTINEL).all() and (s == SENTINEL).all() and (o == SENTINEL).all(), "a store left its output"
        return got


def same_bits(got, want, what):
    data, scl, offs = want
    assert np.array_equal(got[0], data), what + ": bytes"
    assert np.array_equal(got[1], scl.view(np.int32)), what + ": DAT_SCL"
    assert np.array_equal(got[2], offs.view(np.int32)), what + ": DAT_OFFS"


NCHANS = (8, 24, 64, 72, 200)           # one channel tile, a ragged tile, a whole tile, one and a bit, several
NSBLKS = (1, 63, 64, 100, 2048)         # below, at and off the 64-sample tile; many time tiles


@pytest.mark.parametrize("npol", [1, 2, 4])
@pytest.mark.parametrize("nbit", [1, 2, 4, 8])
def test_bit_for_bit_on_exact_data(gpu, nbit, npol):
    """every nchan x nsblk of the tables; rows at odd float offsets with padded strides; flip, swap and both taken in turn"""
    dspsr_amd, ctx = gpu
    rng = np.random.default_rng(SEED + 16 * nbit + npol)
    turn = 0
    for nchan in NCHANS:
        for nsblk in NSBLKS:
            flip, swap = bool(turn & 1), bool(turn & 2)
            offset, pad = (0, 1, 3, 2)[turn % 4], (0, 5, 1)[turn % 3]
            turn += 1
            x = fc.exact_block(rng, nchan, npol, nsblk)
            want = fc.fast_pack(fc.FITSDigitizer(nchan, npol, nbit, nsblk, flip_band=flip, swap_band=swap, row_sums=fc.row_sums_cumsum), x)
            dig = dspsr_amd.FITSDigitizer(ctx, nchan, npol, nbit, nsblk, flip_band=flip, swap_band=swap)
            assert dig.block_bytes == want[0].size and dig.zero_off == 2.0 ** (nbit - 1) - 0.5
            out = Outputs(1, dig.block_bytes, nchan * npol, skew=turn % 3)
            dig.pack(device_rows(x, offset, pad), *out.views(0))
            same_bits(out.collect()[0], want, "nchan %d nsblk %d flip %d swap %d offset %d pad %d" % (nchan, nsblk, flip, swap, offset, pad))
            dig.close()


@pytest.mark.parametrize("nblock,constant", [(1, False), (2, False), (3, False), (1, True), (3, True)])
def test_ring_of_blocks_without_synchronisation(gpu, nblock, constant):
    """2 * nblock + 3 consecutive packs queued with nothing between them: every regime, the ring wrapped twice; `constant`"""
    dspsr_amd, ctx = gpu
    rng = np.random.default_rng(SEED + nblock)
    nchan, npol, nbit, nsblk, n = 72, 2, 4, 100, fc.ring_calls(nblock)
    blocks = [fc.exact_block(rng, nchan, npol, nsblk) for _ in range(n)]
    ref = fc.FITSDigitizer(nchan, npol, nbit, nsblk, nblock=nblock, constant=constant, flip_band=True, row_sums=fc.row_sums_cumsum)
    want = [fc.fast_pack(ref, x) for x in blocks]
    if not constant and nblock > 1:
        assert ref.regimes == ["filling"] * nblock + ["full"] * (nblock + 3)
    rows = [device_rows(x, k % 4, k % 3) for k, x in enumerate(blocks)]
    dig = dspsr_amd.FITSDigitizer(ctx, nchan, npol, nbit, nsblk, nblock=nblock, constant=constant, flip_band=True)
    out = Outputs(n, dig.block_bytes, nchan * npol)
    for k in range(n):
        dig.pack(rows[k], *out.views(k))
    for k, got in enumerate(out.collect()):
        same_bits(got, want[k], "nblock %d constant %d call %d (%s)" % (nblock, constant, k, ref.regimes[k]))
    dig.close()


@pytest.mark.parametrize("nbit", [1, 2, 4, 8])
def test_constant_row_and_huge_values(gpu, nbit):
    """scale 0 -> m_scale inf -> NaN -> INT_MIN -> digi_min; a float square that overflows -> scale inf -> the middle level; an
    outlier at 7.9 sigma -> digi_max: the reference's bits on each"""
    dspsr_amd, ctx = gpu
    x = np.full((8, 1, 64), 37.0, np.float32)
    x[1, 0] = np.arange(64) % 5
    x[2, 0, 7] = 3e38
    x[3, 0, 9] = 1e15
    x[4, 0] = -1200.0
    want = fc.fast_pack(fc.FITSDigitizer(8, 1, nbit, 64, row_sums=fc.row_sums_cumsum), x)
    lev = fc.unpack_levels(want[0], nbit).reshape(64, 8)
    assert (lev[:, 0] == 0).all() and want[1][0] == 0.0 and np.isinf(want[1][2]) and lev[9, 3] >= (1 << nbit) - 2
    dig = dspsr_amd.FITSDigitizer(ctx, 8, 1, nbit, 64)
    out = Outputs(1, dig.block_bytes, 8)
    dig.pack(device_rows(x, 1, 2), *out.views(0))
    same_bits(out.collect()[0], want, "nbit %d" % nbit)
    dig.close()


@pytest.mark.parametrize("nbit", [2, 8])
def test_noise_within_the_licensed_difference(gpu, nbit):
    """Gaussian noise, mean = 10 sigma.  The order of the double sums is the only licensed difference: levels at most 1 apart on at
    most 1e-5 of the samples of a block, DAT_SCL / DAT_OFFS within one float ulp.  At 8 bits every sample whose level lies strictly
    inside (0, 255) decodes to within half a step: |(level - ZERO_OFF) * DAT_SCL + DAT_OFFS - x| <= 0.5 * DAT_SCL * (1 + 2^-20)."""
    dspsr_amd, ctx = gpu
    nchan, npol, nsblk = fc.NOISE_SHAPE
    rng = np.random.default_rng(fc.NOISE_SEED)
    x = fc.noise_block(rng, nchan, npol, nsblk)
    want = fc.fast_pack(fc.FITSDigitizer(nchan, npol, nbit, nsblk, row_sums=fc.row_sums_cumsum), x)
    dig = dspsr_amd.FITSDigitizer(ctx, nchan, npol, nbit, nsblk)
    out = Outputs(1, dig.block_bytes, nchan * npol)
    dig.pack(device_rows(x, 0, 0), *out.views(0))
    data, scl, offs = out.collect()[0]
    lg, lw = fc.unpack_levels(data, nbit), fc.unpack_levels(want[0], nbit)
    d = np.abs(lg - lw)
    ulp_s, ulp_o = np.abs(scl - want[1].view(np.int32)).max(), np.abs(offs - want[2].view(np.int32)).max()
    print("nbit %d: worst level difference %d on %d of %d samples; DAT_SCL %d ulp, DAT_OFFS %d ulp" % (nbit, d.max(), (d != 0).sum(), d.size, ulp_s, ulp_o))
    assert d.max() <= 1 and (d != 0).sum() <= fc.LEVEL_FRACTION * d.size
    assert ulp_s <= 1 and ulp_o <= 1
    if nbit == 8:
        lev = lg.reshape(nsblk, npol, nchan).astype(np.float64)
        s = scl.view(np.float32).astype(np.float64).reshape(1, npol, nchan)
        o = offs.view(np.float32).astype(np.float64).reshape(1, npol, nchan)
        inside = (lev > 0) & (lev < 255)
        err = np.abs((lev - dig.zero_off) * s + o - x.transpose(2, 1, 0).astype(np.float64))
        bound = 0.5 * s * (1 + 2.0 ** -20) * np.ones_like(err)
        print("decoding: %.4f of the samples inside (0, 255); worst error / bound %.6f" % (inside.mean(), (err[inside] / bound[inside]).max()))
        assert inside.mean() >= 0.99 and (err[inside] <= bound[inside]).all()
    dig.close()


def test_two_runs_give_the_same_bytes(gpu):
    dspsr_amd, ctx = gpu
    nchan, npol, nsblk = fc.NOISE_SHAPE
    rng = np.random.default_rng(SEED + 9)
    blocks = [device_rows(fc.noise_block(rng, nchan, npol, nsblk), 1, 1) for _ in range(5)]
    runs = []
    for _ in range(2):
        dig = dspsr_amd.FITSDigitizer(ctx, nchan, npol, 2, nsblk, nblock=2)
        out = Outputs(len(blocks), dig.block_bytes, nchan * npol)
        for k, rows in enumerate(blocks):
            dig.pack(rows, *out.views(k))
        runs.append(out.collect())
        dig.close()
    for a, b in zip(*runs):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_refusals_by_name(gpu):
    """DSPSR_AMD_EINVAL before any launch, the limit named; the outputs keep their sentinel and the next valid call works"""
    dspsr_amd, ctx = gpu
    lib, EINVAL = dspsr_amd.lib, dspsr_amd._lib.EINVAL
    for kw, match in ((dict(nbit=3), "nbit=3 not understood"), (dict(nbit=16), "nbit=16 not understood"), (dict(nbit=0), "nbit=0 not understood"),
                      (dict(nchan=12, nbit=1), "nchan=12 not a multiple of 8 samples per byte"), (dict(nchan=6, nbit=2), "not a multiple of 4"),
                      (dict(nchan=9, nbit=4), "not a multiple of 2"), (dict(nsblk=0), "nsblk == 0"), (dict(nsblk=2 ** 30 + 1), "exceeds 2\\^30 samples"), (dict(nblock=0), "nblock == 0"),
                      (dict(npol=3), "npol=3"), (dict(nchan=0), "nchan=0"), (dict(nchan=16384, npol=4), "nchan\\*npol=65536 exceeds the grid limit")):
        args = {**dict(nchan=8, npol=2, nbit=8, nsblk=64, nblock=1), **kw}
        with pytest.raises(dspsr_amd.DspsrAmdError, match=match):
            dspsr_amd.FITSDigitizer(ctx, **args)
    nchan, npol, nsblk = 8, 2, 64
    rng = np.random.default_rng(SEED + 3)
    x = fc.exact_block(rng, nchan, npol, nsblk)
    rows = device_rows(x, 0, 4)
    dig = dspsr_amd.FITSDigitizer(ctx, nchan, npol, 8, nsblk)
    out = Outputs(1, dig.block_bytes, nchan * npol)
    ob, oscl, ooffs = out.views(0)
    cs, ps = rows.stride(0), rows.stride(1)

    def pack(ptr=rows.data_ptr(), cs=cs, ps=ps, o=ob.data_ptr(), s=oscl.data_ptr(), f=ooffs.data_ptr()):
        rc = lib.dspsr_amd_fits_digitizer_pack(dig.handle, ptr, cs, ps, o, s, f)
        return rc, lib.dspsr_amd_last_error(ctx.handle).decode()

    for kw, match in ((dict(ps=nsblk - 1), "rows of 64 floats overlap"), (dict(cs=ps + nsblk - 1), "rows of 64 floats overlap"), (dict(cs=0), "overlap"),
                      (dict(ptr=rows.data_ptr() + 2), "float aligned"), (dict(s=oscl.data_ptr() + 1), "float aligned"), (dict(ptr=None), "null pointer"),
                      (dict(o=None), "null pointer"), (dict(f=None), "null pointer")):
        rc, msg = pack(**kw)
        assert rc == EINVAL and match in msg, (kw, msg)
    assert lib.dspsr_amd_fits_digitizer_pack(None, rows.data_ptr(), cs, ps, ob.data_ptr(), oscl.data_ptr(), ooffs.data_ptr()) == EINVAL
    with pytest.raises(dspsr_amd.DspsrAmdError, match="one block is"):
        dig.pack(rows[:, :, :nsblk - 1], ob, oscl, ooffs)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="out holds"):
        dig.pack(rows, ob[:-1], oscl, ooffs)
    # nothing was launched and no state moved: the first valid call is the first block
    out.collect()
    dig.pack(rows, ob, oscl, ooffs)
    same_bits(out.collect()[0], fc.fast_pack(fc.FITSDigitizer(nchan, npol, 8, nsblk, row_sums=fc.row_sums_cumsum), x), "after the refusals")
    dig.close()
