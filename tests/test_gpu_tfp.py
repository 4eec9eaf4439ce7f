"""The search-mode front end dspsr_amd_tfp_filterbank (dspsr_amd/csrc/tfp.hip) where a workgroup handles SEVERAL items.  Its three
kernel families are persistent (grid = min(items, compute units)): a workgroup prefetches the first tile of its next item while
it post-processes the last tile of the current one, restarts its running time-scrunch sums per item and hands the LDS image
over between them.  The cases come from tests/tfp_cases.py, the host-side restatement of the launch arithmetic, with the device's
own number of compute units: 2.5 items per workgroup and one more (tests/test_tfp_dispatch_model.py checks, without a GPU, that
every family gets them).

  anchor   the generic kernel with half-word loads at tscrunch 1 against the float64 oracle, every channel count
  exact    every other path == the anchor kernel's per-part powers summed in time order in float32, BIT FOR BIT
  edges    of the entry point: tscrunch 0, npart < tscrunch, refusals, CASPSR blocks off the 16-byte boundary
  chain    LoadToFil with more than two output samples per workgroup in each block

Every run writes into a buffer that holds one NaN bit pattern (tests/device_buffers.py SENTINEL) with rows in front of row 0 and
behind row npart // tscrunch - 1, and reads a block whose buffer holds 0x7f behind it (the kernels' own fill is 0x80)."""
import ctypes as C

import numpy as np
import pytest

import tfp_cases as tc
from device_buffers import SENTINEL

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALE = 0.0123


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count       # what the library's context takes as ncu


def _place(block, align):
    """the block `align` bytes behind a 16-byte boundary, in a buffer whose other bytes (16 or more in front, two tiles behind)
    are 0x7f"""
    n = block.numel()
    buf = torch.full((n + 48 + 2 * tc.TILE_BYTES,), 0x7f, dtype=torch.int8, device="cuda")
    start = (-buf.data_ptr()) % 16 + 16 + align
    raw = buf[start:start + n]
    raw.copy_(block)
    assert raw.data_ptr() % 16 == align % 16
    return raw


def _noise(nbytes, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-128, 128, (nbytes,), dtype=torch.int8, device="cuda", generator=g)


class _Out:
    """[guard rows][nout rows][guard rows] of nchan x npol floats, every float SENTINEL"""

    def __init__(self, nout, nchan, npol):
        self.g = max(3, 16384 // (nchan * npol))
        self.nout = nout
        self.bits = torch.full((2 * self.g + nout, nchan, npol), SENTINEL, dtype=torch.int32, device="cuda")
        self.rows = self.bits[self.g:].view(torch.float32)             # row 0 of the call and everything behind it

    def written(self):
        """the rows of the call, after checking that they are finite and that nothing else changed"""
        g, nout = self.g, self.nout
        assert bool((self.bits[:g] == SENTINEL).all()), "rows in front of row 0 were written"
        tail = self.bits[g + nout:] != SENTINEL
        assert not bool(tail.any()), "rows >= npart // tscrunch were written: first at row %d" % (nout + int(tail.nonzero()[0, 0]))
        w = self.rows[:nout]
        assert bool(torch.isfinite(w).all()), "%d floats of the output not written (or not finite)" % int((~torch.isfinite(w)).sum())
        return w


def _run(gpu, c, block, tscrunch=None, align=None, scale=SCALE):
    dspsr_amd, ctx = gpu
    sf = c.tscrunch if tscrunch is None else tscrunch
    out = _Out(c.npart // max(sf, 1), c.nchan, 1 if c.pscrunch else 2)
    raw = _place(block, c.align if align is None else align)
    dspsr_amd.tfp_filterbank(ctx, raw, c.nchan, c.npart, out.rows, c.pscrunch, sf,
                             layout=dspsr_amd.RAW_CASPSR if c.caspsr else dspsr_amd.RAW_GENERIC, scale=scale)
    torch.cuda.synchronize()
    return out.written()


def _anchor_sums(gpu, c, block, scale=SCALE):
    """the reference of the exact tests: the half-word generic kernel at tscrunch 1, its per-part powers added sequentially in
    float32 in time order (TScrunch.C:193-200: out = in[0]; out += in[1]; ...)"""
    one = _run(gpu, c, block, tscrunch=1, align=tc.half_word_align(c.caspsr), scale=scale)
    sf = c.tscrunch
    nout = c.npart // sf
    seg = one[:nout * sf].view(nout, sf, c.nchan, one.shape[2])
    want = seg[:, 0].clone()
    for i in range(1, sf):
        want += seg[:, i]
    return want


def _assert_same_bits(got, want, c, d):
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    rows = torch.unique(bad[:, 0])
    per_item = d.T // c.tscrunch if c.tscrunch < d.T else 1                    # output samples per work item
    items = torch.unique(rows // per_item)
    raise AssertionError("%s: %d of %d floats differ in %d output samples; first (sample, bin, pol) %s; items %s ... (grid %d of %d items)"
                         % (d.family, len(bad), got.numel(), len(rows), bad[:3].tolist(), items[:8].tolist(), d.grid, d.nitem))


def _oracle_errors(oracle, block, c, got, scale, f32_bins=None):
    """sums of err^2 and want^2, max |err| of `got` against the float64 oracle (TFPFilterbank.C:27-101 + TScrunch.C:180-206 of the
    unpacked block), in chunks of whole output samples; over `f32_bins` alone the same for `got` and for the float32 oracle"""
    obs = oracle.Observation(machine="CASPSR" if c.caspsr else "DADA")
    sf = c.tscrunch
    nout = c.npart // sf
    part_bytes = 4 * c.nchan
    step = max(1, ((16 << 20) // part_bytes) // sf)                  # output samples per chunk
    se = sw = mx = 0.0
    be = bf = bw = 0.0
    for o0 in range(0, nout, step):
        o1 = min(nout, o0 + step)
        un = oracle.unpack_8bit(block[o0 * sf * part_bytes:o1 * sf * part_bytes], obs, scale=scale)
        want = oracle.tscrunch_tfp(oracle.tfp_filterbank(un, c.nchan, c.pscrunch, dtype=np.float64), sf)
        err = got[o0:o1].astype(np.float64) - want
        se, sw, mx = se + float((err * err).sum()), sw + float((want * want).sum()), max(mx, float(np.abs(err).max()))
        if f32_bins is not None:
            assert sf == 1                                            # (tscrunch_tfp with factor 1 copies)
            w32 = oracle.tfp_filterbank(un, c.nchan, c.pscrunch, dtype=np.float32).astype(np.float64)
            be += float((err[:, f32_bins] ** 2).sum())
            bf += float(((w32 - want)[:, f32_bins] ** 2).sum())
            bw += float((want[:, f32_bins] ** 2).sum())
    n = got.size
    nb = n // c.nchan * len(f32_bins) if f32_bins is not None else 1
    return dict(rms_err=(se / n) ** 0.5, rms_want=(sw / n) ** 0.5, max_err=mx,
                bins_rms_err=(be / nb) ** 0.5, bins_rms_f32=(bf / nb) ** 0.5, bins_rms_want=(bw / nb) ** 0.5)


# ---- anchor ------------------------------------------------------------------------------------------------------------------
_ANCHOR = tc.anchor_cases(256)                    # (ids and shapes: the same for every device; npart comes from the device's table)


@pytest.mark.parametrize("i", range(len(_ANCHOR)), ids=[tc.case_id(c) for c in _ANCHOR])
def test_half_word_generic_kernel_against_the_float64_oracle_with_several_items_per_workgroup(oracle, gpu, i):
    """k_tfp with half-word loads (a block 2 bytes behind a 16-byte boundary; CASPSR: 8 bytes) at tscrunch 1, every channel count
    16 ... 8192, 2.5 items per workgroup and a half-filled last tile, against the float64 oracle with the bounds of
    test_tfp_filterbank_search_mode: rms(err) <= 2e-6 rms(want), max |err| <= 1.6e-4 rms(want).

    Bins 0 and nchan / 2 are their own mirrors in the real-transform split and take separate code; an error confined to them
    moves the all-bin rms by 1 / sqrt(nchan) of its size.  So the rms error over bins {0, 1, nchan/2 - 1, nchan/2, nchan/2 + 1,
    nchan - 1} alone is bounded too: by FOUR times the same statistic of the float32 oracle (numpy's float32 pocketfft, then
    Re^2 + Im^2 in float32) against the float64 oracle on the same block -- a radix-16 factorisation with hardware sin / cos in
    the split rounds differently from pocketfft, but not by an order of magnitude.  Measured for the float32 oracle on these
    blocks (numpy 2.2): 5.4e-8 ... 5.7e-8 of the rms of those bins for every channel count, i.e. half an ulp of the float32
    result -- the bound is 2.2e-7 of that rms.  Measured for the kernel on an MI355X: 1.0e-7 ... 1.7e-7 of that rms, 1.8 to 3.0 times
    the float32 oracle's (largest at 64 and 128 channels); all bins: rms 1.0e-7 ... 2.3e-7, max 1.8e-6 ... 5.1e-6 of rms(want).
    The test prints every figure before it asserts."""
    c = tc.anchor_cases(_ncu())[i]
    d = tc.dispatch(c.nchan, 1, c.npart, c.caspsr, c.align, _ncu())
    assert d.family == tc.K_TFP_HALF and d.nitem >= 2 * d.grid + d.grid // 2 + 1
    host = tc.anchor_block(c.nchan, c.npart, 100 + c.nchan + c.caspsr)
    assert host.nbytes <= 64 << 20 or _ncu() > 256
    scale = float(oracle.S8)
    got = _run(gpu, c, torch.from_numpy(host).cuda(), scale=scale).cpu().numpy()
    e = _oracle_errors(oracle, host, c, got, scale, f32_bins=tc.mirror_bins(c.nchan))
    print("anchor %s items %d grid %d: rms err %.3e max err %.3e (of rms want); mirror bins rms err %.3e, float32 oracle %.3e (of their rms)"
          % (tc.case_id(c), d.nitem, d.grid, e["rms_err"] / e["rms_want"], e["max_err"] / e["rms_want"],
             e["bins_rms_err"] / e["bins_rms_want"], e["bins_rms_f32"] / e["bins_rms_want"]))
    assert e["rms_want"] > 0 and e["bins_rms_f32"] > 0
    assert e["rms_err"] <= 2e-6 * e["rms_want"]
    assert e["max_err"] <= 1.6e-4 * e["rms_want"]
    assert e["bins_rms_err"] <= 4.0 * e["bins_rms_f32"]


# ---- exact -------------------------------------------------------------------------------------------------------------------
_EXACT = tc.exact_cases(256)


@pytest.mark.parametrize("i", range(len(_EXACT)), ids=[tc.case_id(c) for c in _EXACT])
def test_every_path_equals_the_anchor_kernel_bit_for_bit_with_several_items_per_workgroup(gpu, i):
    """k_tfp4k, k_tfpm, k_tfp with whole-range loads and k_tfp with half-word loads at tscrunch > 1, each with 2.5 items per
    workgroup: the bits of the anchor kernel's per-part powers summed in time order.  Both byte orders, with and without
    pscrunch, a tail of parts that completes no output sample."""
    ncu = _ncu()
    c = tc.exact_cases(ncu)[i]
    d = tc.dispatch(c.nchan, c.tscrunch, c.npart, c.caspsr, c.align, ncu)
    assert d.nitem >= 2 * ncu + 1 and d.grid == ncu
    block = _noise(c.npart * 4 * c.nchan, 1000 + i)
    want = _anchor_sums(gpu, c, block)
    got = _run(gpu, c, block)
    _assert_same_bits(got, want, c, d)
    assert float(got.min()) >= 0.0 and float(got.max()) > 0.0


def test_benchmark_geometry_eight_items_per_workgroup(oracle, gpu):
    """digifil -F 4096 -t 16 on 16 * 8 * ncu parts (the benchmark's 32768 on 256 compute units): k_tfp4k, eight output samples of
    eight tiles per workgroup -- the anchor kernel's sums bit for bit, and the float64 oracle with the anchor's bounds."""
    ncu = _ncu()
    c = tc.bench_case(ncu)
    d = tc.dispatch(c.nchan, c.tscrunch, c.npart, c.caspsr, c.align, ncu)
    assert (d.family, d.groups_per_out, d.nitem, d.grid) == (tc.K_TFP4K, 8, 8 * ncu, ncu)
    scale = float(oracle.S8)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    nbytes = c.npart * 4 * c.nchan
    block = torch.empty(nbytes, dtype=torch.int8, device="cuda")
    for b0 in range(0, nbytes, 1 << 26):                               # Gaussian of 24 levels rms, clipped
        n = min(1 << 26, nbytes - b0)
        block[b0:b0 + n] = torch.clamp(torch.round(torch.randn(n, device="cuda", generator=g) * 24.0), -128, 127).to(torch.int8)
    want = _anchor_sums(gpu, c, block, scale=scale)
    got = _run(gpu, c, block, scale=scale)
    _assert_same_bits(got, want, c, d)
    del want
    e = _oracle_errors(oracle, block.cpu().numpy(), c, got.cpu().numpy(), scale)
    print("bench geometry, %d items on %d workgroups: rms err %.3e max err %.3e (of rms want)"
          % (d.nitem, d.grid, e["rms_err"] / e["rms_want"], e["max_err"] / e["rms_want"]))
    assert e["rms_want"] > 0
    assert e["rms_err"] <= 2e-6 * e["rms_want"]
    assert e["max_err"] <= 1.6e-4 * e["rms_want"]


# ---- edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan,caspsr,pscrunch,align", [(64, False, True, 0), (64, True, False, 8), (4096, False, False, 0),
                                                         (8192, True, True, 0), (1024, False, True, 2)])
def test_tscrunch_0_means_1(gpu, nchan, caspsr, pscrunch, align):
    ncu = _ncu()
    c = tc.Case(nchan, 0, caspsr, pscrunch, tc.npart_for(nchan, 1, ncu + 3), align)
    block = _noise(c.npart * 4 * nchan, 7)
    got0, got1 = _run(gpu, c, block, tscrunch=0), _run(gpu, c, block, tscrunch=1)
    assert got0.shape[0] == c.npart and torch.equal(got0, got1) and float(got1.max()) > 0.0


@pytest.mark.parametrize("nchan,tscrunch,npart,caspsr,align", [(4096, 16, 15, False, 0), (512, 32, 31, True, 0), (64, 256, 255, False, 2),
                                                               (8192, 3, 2, True, 8), (16, 4, 0, False, 0)])
def test_fewer_parts_than_tscrunch_writes_nothing(gpu, nchan, tscrunch, npart, caspsr, align):
    dspsr_amd, ctx = gpu
    assert tc.dispatch(nchan, tscrunch, npart, caspsr, align, _ncu()) == tc.Dispatch(None, 8192 // nchan, 0, 0, 0, 0, None)
    c = tc.Case(nchan, tscrunch, caspsr, False, npart, align)
    got = _run(gpu, c, _noise(max(npart, 1) * 4 * nchan, 8))            # returns OK; _Out.written(): every float still SENTINEL
    assert got.shape[0] == 0


def test_refused_calls_say_why_and_write_nothing(gpu):
    """EINVAL with the text of tests/tfp_cases.py dispatch() (the model restates the library's checks in their order), nothing
    launched.  An odd pointer is refused for BOTH byte orders: tfp_word reads half words -- the (p0, p1) pair of a sample in the
    generic order, two consecutive samples of one polarisation in a CASPSR group -- and a CASPSR stream moves by groups of 8."""
    dspsr_amd, ctx = gpu
    from dspsr_amd import _lib
    block = _noise(64 * 4 * 16384 + 64, 9)
    for nchan, sf, npol, caspsr, align in ((4096, 3, 2, False, 0), (512, 24, 2, True, 0), (16, 768, 2, False, 0), (2048, 6, 2, False, 2),
                                           (64, 1, 2, False, 1), (64, 16, 2, False, 7), (64, 1, 2, True, 1), (4096, 16, 2, True, 9),
                                           (8, 1, 2, False, 0), (16384, 1, 2, False, 0), (48, 1, 2, False, 0),
                                           (64, 1, 1, False, 0), (64, 1, 4, True, 0)):
        d = tc.dispatch(nchan, sf, 64, caspsr, align, _ncu(), npol=npol)
        assert d.family is None and d.refused
        out = _Out(64 // sf, max(nchan, 16), 2)
        raw = _place(block[:64 * 4 * nchan], align)
        cfg = _lib.TfpConfig(nchan, npol, 0, sf)
        code = _lib.lib.dspsr_amd_tfp_filterbank(ctx.handle, C.byref(cfg), raw.data_ptr(), _lib.RAW_CASPSR if caspsr else _lib.RAW_GENERIC,
                                                 SCALE, out.rows.data_ptr(), 64)
        text = _lib.lib.dspsr_amd_last_error(ctx.handle).decode()
        torch.cuda.synchronize()
        assert code == _lib.EINVAL and text == "dspsr_amd_tfp_filterbank: " + d.refused, (nchan, sf, npol, caspsr, align, code, text)
        assert bool((out.bits == SENTINEL).all()), (nchan, sf, npol, caspsr, align)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="unknown raw layout 2"):
        dspsr_amd.tfp_filterbank(ctx, block, 64, 64, _Out(64, 64, 2).rows, False, 1, layout=_lib.RAW_UWB16)


_OFFSETS = tc.caspsr_offset_cases(256)


@pytest.mark.parametrize("i", range(len(_OFFSETS)), ids=[tc.case_id(c) for c in _OFFSETS])
def test_caspsr_blocks_off_the_16_byte_boundary_give_the_bits_of_the_aligned_block(gpu, i):
    """a CASPSR block 2, 4 or 8 bytes behind a 16-byte boundary (the half-word kernel) == the same bytes on the boundary
    (k_tfp4k, k_tfpm, k_tfp with whole-range loads), 2.5 items per workgroup"""
    ncu = _ncu()
    c = tc.caspsr_offset_cases(ncu)[i]
    d = tc.dispatch(c.nchan, c.tscrunch, c.npart, True, 0, ncu)
    assert tc.dispatch(c.nchan, c.tscrunch, c.npart, True, c.align, ncu).family == tc.K_TFP_HALF and d.family != tc.K_TFP_HALF
    block = _noise(c.npart * 4 * c.nchan, 2000 + i)
    _assert_same_bits(_run(gpu, c, block, align=0), _run(gpu, c, block), c, d)


# ---- chain -------------------------------------------------------------------------------------------------------------------
def test_load_to_fil_matches_oracle_chain_with_several_output_samples_per_workgroup(oracle, gpu):
    """test_load_to_fil_matches_oracle_chain (tests/test_gpu_parity.py) at a block size that gives every workgroup of the front end
    more than two output samples: TFPFilterbank (PPQQ) -> TScrunch -> Rescale -> PScrunch -> SigProcDigitizer, 8 bit, three
    blocks.  Bytes at most one level apart, in fewer than 1e-3 of the samples."""
    dspsr_amd, _ = gpu
    from dspsr_amd import pipeline
    o = oracle
    ncu = _ncu()
    nchan, tscr, npart = tc.chain_case(ncu)
    d = tc.dispatch(nchan, tscr, npart, False, 0, ncu)
    assert d.family == tc.K_TFPM and d.nout > 2 * ncu and d.nitem == d.nout
    info = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=400.0, tsamp_us=0.00125, machine="DADA")
    cfg = pipeline.SearchConfig(nchan=nchan, tscrunch=tscr, nbit=8, rescale_seconds=10.0, parts_per_block=npart)
    lf = pipeline.LoadToFil(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
    obs = o.Observation()
    ro = o.Rescale(int(10.0 * lf.out_rate), False)
    worst, frac = 0, 0.0
    for b in range(3):
        raw = tc.anchor_block(nchan, npart, 60 + b)
        dev = torch.from_numpy(raw).cuda()
        assert dev.data_ptr() % 16 == 0                                # (whole-range loads: the register-split kernel)
        got = lf.process_block(dev).cpu().numpy()
        det = ro.transform(o.tscrunch_tfp(o.tfp_filterbank(o.unpack_8bit(raw, obs), nchan, False), tscr))
        want = o.sigproc_digitize(o.pscrunch_tfp(det), 8, use_digi_scales=True, flip_band=True)
        assert got.size == want.size == d.nout * nchan
        dl = np.abs(got.reshape(-1).astype(np.int32) - want.reshape(-1).astype(np.int32))
        worst, frac = max(worst, int(dl.max())), max(frac, float((dl != 0).mean()))
    print("chain at scale: %d output samples per block on %d workgroups, worst %d level, %.2e of the samples" % (d.nout, d.grid, worst, frac))
    assert worst <= 1 and frac < 1e-3
    lf.close()
