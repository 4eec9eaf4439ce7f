"""MeerKAT heaps (DSPSR_AMD_RAW_MEERKAT / _SWAP) on the device: the unpacker k_unpack_heaps bit for bit against the loop restatement
of tests/heap_cases.py, on rows cut from sentinel buffers; and the heap loader of the one-pass convolution (k_conv1_heaps, one case per
instantiation) bit for bit against unpack-then-convolve on the same object, against the float64 oracle, through every raw entry
point, with the refusals of the objects that have no such loader."""
import ctypes as C
import math

import numpy as np
import pytest

import heap_cases as hc
from device_buffers import SENTINEL, OutputLayout, describe_float, place_parts, sentinel_rows

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


def _layout(dspsr_amd, machine, first=0):
    base = dspsr_amd.RAW_MEERKAT_SWAP if hc.MACHINES[machine] else dspsr_amd.RAW_MEERKAT
    return dspsr_amd.raw_at(base, first)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ---- the unpacker ------------------------------------------------------------------------------------------------------------------
WINDOWS = [(0, 256), (0, 513), (1, 255), (255, 2), (37, 1000)]          # (first_sample, ndat)


@pytest.mark.parametrize("machine", sorted(hc.MACHINES))
@pytest.mark.parametrize("npol", [1, 2])
@pytest.mark.parametrize("nchan", [1, 3, 64])
def test_unpack_heaps_bit_for_bit(gpu, nchan, npol, machine):
    """every window at every row offset 0-3 (floats past a 256-byte boundary), the paddings 0, 1 and 3 in turn: the rows hold the
    restatement's bits and no other float of the buffer is touched"""
    dspsr_amd, ctx = gpu
    swap = hc.MACHINES[machine]
    scale = float(dspsr_amd.eight_bit_scale())
    nheap = 5
    block = hc.random_block(nheap, nchan, npol, seed=nchan + npol)
    stream = hc.stream_from_heaps(block, nchan, npol, swap)
    d_block = torch.from_numpy(block).cuda()
    assert d_block.data_ptr() % 16 == 0
    k = 0
    for first, ndat in WINDOWS:
        want = hc.rows_of(stream, first, ndat, scale)
        for offset in range(4):
            pad = (0, 1, 3)[k % 3]
            k += 1
            lay = OutputLayout(nchan, npol, 2 * ndat, offset=offset, row_pad=pad)
            buf, rows = sentinel_rows(lay)
            nheap_call = -(-(first + ndat) // 256)
            dspsr_amd.unpack_heaps_fpt(ctx, d_block[:hc.heap_bytes(nheap_call, nchan, npol)], rows, nchan, npol, _layout(dspsr_amd, machine, first),
                                       scale, ndat=ndat)
            ctx.synchronize()
            got = buf.cpu().numpy()
            exp = place_parts(lay, np.full(lay.size, SENTINEL, np.int32), want.view(np.int32).reshape(nchan, npol, 1, 2 * ndat), 0)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, "%s nchan %d npol %d first %d ndat %d offset %d pad %d: %d floats differ, the first: %s" % (
                machine, nchan, npol, first, ndat, offset, pad, bad.size, describe_float(lay, int(bad[0]), 1, 0, 2 * ndat))


def test_unpack_heaps_empty_call_and_refusals(gpu):
    dspsr_amd, ctx = gpu
    from dspsr_amd import _lib
    nchan, npol = 3, 2
    block = torch.from_numpy(hc.random_block(3, nchan, npol)).cuda()
    ndat = 300
    lay = OutputLayout(nchan, npol, 2 * ndat)
    buf, rows = sentinel_rows(lay)
    ocs, ops = rows.stride(0), rows.stride(1)

    def call(raw_ptr, layout, npol_=npol, n=ndat, cs=ocs, ps=ops):
        return _lib.lib.dspsr_amd_unpack_heaps_fpt(ctx.handle, raw_ptr, layout, 1.0, nchan, npol_, n, rows.data_ptr(), cs, ps)

    def message():
        return _lib.lib.dspsr_amd_last_error(ctx.handle).decode()

    ptr = block.data_ptr()
    assert call(ptr, _lib.RAW_MEERKAT, n=0) == _lib.OK                                   # ndat = 0: nothing to do
    assert call(ptr + 1, _lib.RAW_MEERKAT) == _lib.EINVAL and "16 bytes" in message()    # odd
    assert call(ptr + 8, _lib.RAW_MEERKAT_SWAP) == _lib.EINVAL and "16 bytes" in message()
    assert call(ptr, _lib.RAW_MEERKAT, cs=ops) == _lib.EINVAL and "overlap" in message()   # channel rows inside each other
    assert call(ptr, _lib.RAW_MEERKAT, ps=2 * ndat - 2) == _lib.EINVAL and "overlap" in message()
    assert call(ptr, _lib.RAW_MEERKAT, npol_=4) == _lib.EINVAL and "npol" in message()
    assert call(ptr, _lib.RAW_MEERKAT | (256 << 8)) == _lib.EINVAL and "first_sample" in message()
    assert call(ptr, _lib.RAW_GENERIC) == _lib.EINVAL and call(ptr, _lib.RAW_GENERIC | (1 << 8)) == _lib.EINVAL
    ctx.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused or empty call wrote"


# ---- the heap loader of the one-pass convolution ------------------------------------------------------------------------------
NCHAN = 3           # the run stride of a polarisation is 3 * 512 bytes


def _conv_case(M):
    """(nfilt, npart, max_parts): nsamp_step odd, so that parts start at every phase of a heap; a ragged last tile of the 2^13-point
    tile (Ts = 2^12 / M parts of two polarisations) for M <= 2048, three parts above"""
    nfilt = (M // 8 + 1, M // 16)
    assert (M - sum(nfilt)) % 2 == 1
    Ts = (1 << 12) // M if M <= 4096 else 1
    return nfilt, (Ts + 1 if M <= 2048 else 3), 2


class _Case:
    pass


@pytest.fixture(scope="module")
def conv_cases(gpu, oracle):
    """per M: the block of heaps, the response, and one fused and one unfused engine (built on first use, closed at the end)"""
    dspsr_amd, ctx = gpu
    made = {}

    def get(M):
        if M in made:
            return made[M]
        c = _Case()
        c.M = M
        c.nfilt, c.npart, c.max_parts = _conv_case(M)
        c.step = M - sum(c.nfilt)
        c.nsamp = c.npart * c.step + sum(c.nfilt)
        rng = np.random.default_rng(M)
        c.kernel = np.exp(1j * rng.uniform(-np.pi, np.pi, NCHAN * M)).astype(np.complex64)
        c.nheap = -(-(255 + c.nsamp) // 256)
        c.block = hc.random_block(c.nheap, NCHAN, 2, seed=M + 1)
        c.d_block = torch.from_numpy(c.block).cuda()
        c.streams = {}
        c.fused = dspsr_amd.FilterbankEngine(ctx).setup(1, M, c.nfilt[0], c.nfilt[1], NCHAN, 2, False, c.kernel, max_parts=c.max_parts)
        c.unfused = dspsr_amd.FilterbankEngine(ctx).setup(1, M, c.nfilt[0], c.nfilt[1], NCHAN, 2, False, c.kernel, max_parts=c.max_parts,
                                                          fuse_heaps=False)
        made[M] = c
        return c
    yield get
    for c in made.values():
        c.fused.close()
        c.unfused.close()


def _stream(c, machine):
    if machine not in c.streams:
        c.streams[machine] = hc.stream_from_heaps(c.block, NCHAN, 2, hc.MACHINES[machine])
    return c.streams[machine]


@pytest.mark.parametrize("machine", sorted(hc.MACHINES))
@pytest.mark.parametrize("first", [0, 1, 255])
@pytest.mark.parametrize("M", [64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_heap_loader_equals_unpack_then_convolve(gpu, oracle, conv_cases, M, first, machine):
    dspsr_amd, ctx = gpu
    c = conv_cases(M)
    scale = float(dspsr_amd.eight_bit_scale())
    layout = _layout(dspsr_amd, machine, first)
    npart, step, nkeep = c.npart, c.step, c.step
    assert c.fused.takes_heaps() and c.unfused.takes_heaps() and c.fused.npass(False) == 1
    assert (c.fused.nsamp_step, c.fused.nkeep) == (step, nkeep)
    nheap = -(-(first + c.nsamp) // 256)
    raw = c.d_block[:hc.heap_bytes(nheap, NCHAN, 2)]
    # the float rows: unpack_heaps_fpt, which must be the restatement's floats
    x = torch.zeros((NCHAN, 2, 2 * c.nsamp), dtype=torch.float32, device="cuda")
    dspsr_amd.unpack_heaps_fpt(ctx, raw, x, NCHAN, 2, layout, scale, ndat=c.nsamp)
    want_x = hc.rows_of(_stream(c, machine), first, c.nsamp, scale)
    assert _same_bits(x.cpu().numpy(), want_x)

    # complex rows: float entry point on the unpacked rows == heap block, fused and unfused; nothing outside the rows written
    lay = OutputLayout(NCHAN, 2, 2 * npart * nkeep, offset=2, row_pad=3)
    outs = []
    for how in ("float", "fused", "unfused"):
        buf, rows = sentinel_rows(lay)
        if how == "float":
            c.fused.perform(x, rows, npart, 2 * step, 2 * nkeep)
        else:
            (c.fused if how == "fused" else c.unfused).perform_raw(raw, layout, scale, rows, npart)
        ctx.synchronize()
        outs.append(buf.cpu().numpy())
    got = outs[0][lay.first:lay.first + NCHAN * 2 * (lay.row + lay.row_pad)].view(np.float32).reshape(NCHAN, 2, -1)[:, :, :lay.row]
    mask = place_parts(lay, np.zeros(lay.size, np.int32), np.ones((NCHAN, 2, 1, lay.row), np.int32), 0).astype(bool)
    for name, o_ in zip(("float", "fused", "unfused"), outs):
        assert bool((o_[~mask] == SENTINEL).all()), "%s wrote outside the rows" % name
        assert np.array_equal(o_, outs[0]), "perform_raw (%s) differs from unpack + perform" % name

    # the float64 oracle on the restatement's floats
    ref = oracle.convolution(want_x, M, c.nfilt[0], c.nfilt[1], c.kernel, False, npart=npart, dtype=np.float64)
    rms = math.sqrt(np.mean(np.abs(ref) ** 2))
    tol = 2e-6 * math.sqrt(math.log2(2 * M))
    gc = np.ascontiguousarray(got).view(np.complex64).astype(np.complex128)
    err_rms, err_max = math.sqrt(np.mean(np.abs(gc - ref) ** 2)) / rms, np.abs(gc - ref).max() / rms
    print("M", M, "rms error", err_rms, "largest", err_max, "bounds", tol, 8 * tol)
    assert err_rms <= tol
    assert err_max <= 8 * tol

    # detected rows, every layout and both states
    for state_name, state in (("Coherence", dspsr_amd.COHERENCE), ("Stokes", dspsr_amd.STOKES)):
        prod = oracle.detect_products(ref, state_name)
        for ndim in (1, 2, 4):
            want = oracle.detect_layout(prod, ndim).reshape(NCHAN, 4 // ndim, -1)
            dlay = OutputLayout(NCHAN, 4 // ndim, npart * nkeep * ndim, offset=1, row_pad=1)
            dets = []
            for how in ("float", "fused", "unfused"):
                buf, rows = sentinel_rows(dlay)
                if how == "float":
                    c.fused.perform_detect(rows, npart, state, ndim, inp=x, in_step=2 * step)
                else:
                    (c.fused if how == "fused" else c.unfused).perform_detect(rows, npart, state, ndim, raw=raw, layout=layout, scale=scale)
                ctx.synchronize()
                dets.append((buf.cpu().numpy(), rows.cpu().numpy()))
            dmask = place_parts(dlay, np.zeros(dlay.size, np.int32), np.ones((NCHAN, 4 // ndim, 1, dlay.row), np.int32), 0).astype(bool)
            for name, (b_, _r) in zip(("float", "fused", "unfused"), dets):
                assert bool((b_[~dmask] == SENTINEL).all()), "%s ndim %d: %s wrote outside the rows" % (state_name, ndim, name)
                assert np.array_equal(b_, dets[0][0]), "%s ndim %d: perform_detect (%s) differs from unpack + perform_detect" % (state_name, ndim, name)
            assert np.abs(dets[1][1] - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("machine", sorted(hc.MACHINES))
@pytest.mark.parametrize("M", [256, 4096])
def test_fold_and_search_on_heaps_equal_the_unpacked_rows(gpu, conv_cases, M, machine):
    """a 2-part call and then a 3-part call that continues the stream (it starts inside a heap and, for the search, with a carry):
    perform_fold and perform_search on the heap blocks == the same calls on the unpacked rows, bit for bit, fused and unfused"""
    dspsr_amd, ctx = gpu
    M_case = conv_cases(M)
    nfilt, step = M_case.nfilt, M_case.step
    calls, first0 = (2, 3), 200
    nsamp_all = sum(calls) * step + sum(nfilt)
    nheap_all = -(-(first0 + nsamp_all) // 256)
    block = hc.random_block(nheap_all, NCHAN, 2, seed=M + 7)
    d_block = torch.from_numpy(block).cuda()
    scale = float(dspsr_amd.eight_bit_scale())
    nbin, ts = 16, 7
    assert (calls[0] * step) % ts != 0 and (first0 + calls[0] * step) % 256 != 0
    engs = {"float": dspsr_amd.FilterbankEngine(ctx).setup(1, M, nfilt[0], nfilt[1], NCHAN, 2, False, M_case.kernel, max_parts=2),
            "fused": dspsr_amd.FilterbankEngine(ctx).setup(1, M, nfilt[0], nfilt[1], NCHAN, 2, False, M_case.kernel, max_parts=2),
            "unfused": dspsr_amd.FilterbankEngine(ctx).setup(1, M, nfilt[0], nfilt[1], NCHAN, 2, False, M_case.kernel, max_parts=2, fuse_heaps=False)}
    results = {}
    for how, eng in engs.items():
        fold = dspsr_amd.FoldEngine(ctx)
        fold.set_shape(NCHAN, 1, 4, nbin)
        fold.set_nbin(nbin)
        carry = torch.zeros((NCHAN, 2), dtype=torch.float32, device="cuda")
        cc, pos, scr = 0, 0, []
        for npart in calls:
            s0 = first0 + pos * step
            first, h0 = s0 & 255, s0 >> 8
            nsamp = npart * step + sum(nfilt)
            raw = d_block[hc.heap_bytes(h0, NCHAN, 2):hc.heap_bytes(h0 + -(-(first + nsamp) // 256), NCHAN, 2)]
            layout = _layout(dspsr_amd, machine, first)
            ndat = npart * step
            fold.set_ndat(ndat, 0)
            fold.set_bins(0.1 + 0.013 * pos, 0.0137, ndat, 0, np.zeros(nbin, np.uint32))
            lay = OutputLayout(NCHAN, 2, (cc + ndat) // ts, offset=3, row_pad=1)
            buf, out = sentinel_rows(lay)
            if how == "float":
                x = torch.zeros((NCHAN, 2, 2 * nsamp), dtype=torch.float32, device="cuda")
                dspsr_amd.unpack_heaps_fpt(ctx, raw, x, NCHAN, 2, layout, scale, ndat=nsamp)
                eng.perform_fold(fold, npart, dspsr_amd.STOKES, inp=x, in_step=2 * step)
                nout, cc = eng.perform_search(out, carry, cc, npart, ts, dspsr_amd.PPQQ, inp=x, in_step=2 * step)
            else:
                eng.perform_fold(fold, npart, dspsr_amd.STOKES, raw=raw, layout=layout, scale=scale)
                nout, cc = eng.perform_search(out, carry, cc, npart, ts, dspsr_amd.PPQQ, raw=raw, layout=layout, scale=scale)
            ctx.synchronize()
            assert nout == lay.row
            scr.append(buf.cpu().numpy())
            pos += npart
        results[how] = (fold.synch().copy(), scr, carry.cpu().numpy(), cc)
        fold.close()
        eng.close()
    ref = results["float"]
    assert np.abs(ref[0]).max() > 0 and ref[3] == (sum(calls) * step) % ts
    for how in ("fused", "unfused"):
        got = results[how]
        assert _same_bits(got[0], ref[0]), "%s: folded profile differs" % how
        assert all(np.array_equal(a, b) for a, b in zip(got[1], ref[1])), "%s: scrunched rows (or the floats around them) differ" % how
        assert _same_bits(got[2], ref[2]) and got[3] == ref[3]


def test_objects_without_the_loader_refuse_heaps_by_name(gpu):
    dspsr_amd, ctx = gpu
    from dspsr_amd import _lib
    rng = np.random.default_rng(3)
    block = torch.from_numpy(hc.random_block(600, 3, 2)).cuda()

    def message():
        return _lib.lib.dspsr_amd_last_error(ctx.handle).decode()

    def perform_raw(eng, layout, raw=block):
        out = torch.zeros((eng.cfg.input_nchan * eng.cfg.nchan_subband, eng.cfg.npol, 2 * eng.nkeep), dtype=torch.float32, device="cuda")
        return _lib.lib.dspsr_amd_filterbank_perform_raw(eng.handle, raw.data_ptr(), layout, 1.0, out.data_ptr(), out.stride(0), out.stride(1), 1,
                                                         2 * eng.nkeep)

    # (nchan_subband, freq_res, input_nchan, npol, force_four_pass) and the word of the limit the message must name
    for (nsub, M, nchan, npol, ffp), word in (((1, 16384, 3, 2, 0), "freq_res=16384"), ((4, 1024, 3, 2, 0), "nchan_subband=4"),
                                              ((1, 1024, 3, 1, 0), "npol=1"), ((1, 1024, 3, 2, 1), "force_four_pass=1")):
        kernel = np.exp(1j * rng.uniform(-np.pi, np.pi, nchan * nsub * M)).astype(np.complex64)
        eng = dspsr_amd.FilterbankEngine(ctx).setup(nsub, M, M // 8, M // 16, nchan, npol, False, kernel, force_four_pass=ffp)
        assert not eng.takes_heaps()
        for layout in (_lib.RAW_MEERKAT, _lib.raw_at(_lib.RAW_MEERKAT_SWAP, 5)):
            assert perform_raw(eng, layout) == _lib.EINVAL
            assert "takes_heaps" in message() and word in message(), message()
        eng.close()
    M = 1024
    kernel = np.exp(1j * rng.uniform(-np.pi, np.pi, 3 * M)).astype(np.complex64)
    eng = dspsr_amd.FilterbankEngine(ctx).setup(1, M, M // 8, M // 16, 3, 2, False, kernel)
    assert eng.takes_heaps()
    assert perform_raw(eng, _lib.RAW_GENERIC | (1 << 8)) == _lib.EINVAL and "first_sample" in message()     # DSPSR_AMD_RAW_AT(GENERIC, 1)
    assert perform_raw(eng, _lib.RAW_MEERKAT | (256 << 8)) == _lib.EINVAL and "first_sample" in message()
    assert perform_raw(eng, _lib.RAW_MEERKAT, block[8:]) == _lib.EINVAL and "16 bytes" in message()
    assert perform_raw(eng, _lib.RAW_MEERKAT, block[1:]) == _lib.EINVAL and "16 bytes" in message()
    assert perform_raw(eng, _lib.RAW_MEERKAT) == _lib.OK
    ctx.synchronize()
    eng.close()
