"""pipeline.LoadToFITS (digifits, Signal/General/LoadToFITS.C) on the device: its blocks equal dspsr_amd.FITSDigitizer applied by hand to
the rows that the already-tested detect_scrunch of LoadToFilCoherent / LoadToFilDirect yields for the same stream (bit for bit, -K
included); every split of the stream into calls gives the same file; the tool writes that file; a dispersed pulse arrives where the
dispersion law says once -do_dedisp is on."""
import math
import os
import sys

import numpy as np
import pytest

import fits_cases as fc
import heap_cases as hc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSBLK = 128
DM_CONST = 2.41e-4

# the three inputs.  `front`: what the reference chain is built from by hand (class, SearchConfig fields); `parts`: two ways to cut
# the stream into calls -- one call, and unequal calls of which the first completes no block and one completes at least three
SHAPES = {
    # 8-bit real dual-polarisation single-channel input at 32 MHz, digifits -F 16:D -x 256 -D 1 -do_dedisp true -t 16e-6: the minimum
    # transform of this response is 8 points, -x 256 makes it 2048 (LoadToFITS.C:272); 2044 samples kept per part, tscrunch 16:
    # 127.75 output samples per part
    "real": dict(info=dict(centre_frequency=1400.0, bandwidth=-16.0, nchan=1, npol=2, ndim=1, tsamp_us=1.0 / 32.0, machine="DADA"),
                 fits=dict(nchan=16, convolve=True, freq_res=256, dispersion_measure=1.0, coherent_dedisp=True, tsamp=16e-6, parts_per_block=14),
                 front=("LoadToFilCoherent", dict(nchan=16, dispersion_measure=1.0, freq_res=2048, tscrunch=16, parts_per_block=14)),
                 tres=16, out_rate=62500.0, parts=((14,), (1, 5, 2, 6)), swap=dict(swap=False, nsub_swap=0)),
    # a 4-channel complex file at 1 MHz per channel with no -F, digifits -t 16e-6 [-D 100 -K]
    "direct": dict(info=dict(centre_frequency=1400.0, bandwidth=4.0, nchan=4, npol=2, ndim=2, tsamp_us=1.0, machine="DADA"),
                   fits=dict(nchan=0, dispersion_measure=100.0, tsamp=16e-6, parts_per_block=16384),
                   front=("LoadToFilDirect", dict(tscrunch=16, parts_per_block=16384)),
                   tres=16, out_rate=62500.0, parts=((12988,), (100, 7000, 1, 0, 5887)), swap=dict(swap=False, nsub_swap=0)),
    # an MKBFRo file of 4 channels at 4 MHz each through -F 4:D -x 1 -D 10 -do_dedisp true -t 4e-6: 1024-point transforms (the heap
    # loader's), 462 samples kept per part; the reference's tres_factor counts the per-channel rate against all 4 channels:
    # round(16 / 4) = 4, so the chain delivers 1 us samples (TBIN) where the reference prints 4 us
    "heaps": dict(info=dict(centre_frequency=1382.0, bandwidth=-16.0, nchan=4, npol=2, ndim=2, tsamp_us=0.25, machine="MKBFRo"),
                  fits=dict(nchan=4, convolve=True, freq_res=1, dispersion_measure=10.0, coherent_dedisp=True, tsamp=4e-6, parts_per_block=12, max_parts=2),
                  front=("LoadToFilCoherent", dict(nchan=4, dispersion_measure=10.0, freq_res=1024, tscrunch=4, parts_per_block=12, max_parts=2)),
                  tres=4, out_rate=1e6, parts=((12,), (1, 4, 2, 5)), swap=dict(swap=False, nsub_swap=4)),
}

# shape, -p, -b, -K, -I / -c
RUNS = [("real", 1, 8, False, {}), ("real", 2, 2, False, dict(rescale_seconds=0.004)), ("real", 4, 4, False, {}), ("real", 1, 1, True, {}),
        ("direct", 1, 4, False, dict(rescale_constant=True)), ("direct", 2, 8, False, {}), ("direct", 4, 2, True, {}), ("direct", 1, 8, True, {}),
        ("heaps", 1, 2, False, {}), ("heaps", 2, 4, False, dict(rescale_seconds=0.0015)), ("heaps", 4, 8, False, {}), ("heaps", 2, 8, True, {})]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


_streams = {}


def stream_of(name):
    """(raw int8 stream in file order, (step, overlap) of the front end in samples -- None without -F), made once"""
    if name in _streams:
        return _streams[name]
    from dspsr_amd import dada, pipeline
    s = SHAPES[name]
    info = pipeline.InputInfo(**s["info"])
    rng = np.random.default_rng(20151124 + len(name))
    if name == "direct":
        ndat = sum(s["parts"][0])
        raw = np.clip(np.rint(rng.normal(0.0, 24.0, ndat * 4 * 2 * 2)), -128, 127).astype(np.int8)
        _streams[name] = (raw, None)
        return _streams[name]
    cls, kw = s["front"]
    r = pipeline.matched_response(info, kw["dispersion_measure"], kw["freq_res"], kw["nchan"], input_nchan=info.nchan, ndim=info.ndim)
    assert r.ndat == kw["freq_res"]
    nsub = kw["nchan"] // info.nchan
    per = (2 if info.ndim == 1 else 1) * nsub                    # input samples per sample of a filterbank channel
    step, ovl = (r.ndat - r.impulse_pos - r.impulse_neg) * per, (r.impulse_pos + r.impulse_neg) * per
    ndat = sum(s["parts"][0]) * step + ovl
    if name == "heaps":
        ndat += (-ndat) % hc.HEAP
        tfp = np.clip(np.rint(rng.normal(0.0, 24.0, (ndat, 4, 2, 2))), -128, 127).astype(np.int8)
        raw = dada.heaps_from_tfp(tfp, True).reshape(-1)
    else:
        raw = np.clip(np.rint(rng.normal(0.0, 24.0, ndat * 2)), -128, 127).astype(np.int8)
    _streams[name] = (raw, (step, ovl))
    return _streams[name]


def calls_of(name, parts):
    """the arguments of process_block / detect_scrunch for the stream cut into `parts`: (host bytes, npart or ndat[, first_sample])"""
    raw, geom = stream_of(name)
    info = SHAPES[name]["info"]
    bps = info["nchan"] * info["npol"] * info["ndim"]
    out, s0 = [], 0
    for n in parts:
        if geom is None:
            out.append((raw[s0 * bps:(s0 + n) * bps], n))
            s0 += n
            continue
        step, ovl = geom
        nsamp = n * step + ovl
        if name == "heaps":
            first, hb = s0 % hc.HEAP, bps * hc.HEAP
            h0, nheap = s0 // hc.HEAP, -(-(first + nsamp) // hc.HEAP)
            out.append((raw[h0 * hb:(h0 + nheap) * hb], n, first))
        else:
            out.append((raw[s0 * bps:(s0 + nsamp) * bps], n))
        s0 += n * step
    return out


def fits_config(pipeline, name, npol, nbit, dedisperse, extra):
    return pipeline.FitsConfig(**{**SHAPES[name]["fits"], **extra}, npol=npol, nbit=nbit, nsblk=NSBLK, dedisperse=dedisperse)


def run_fits(pipeline, name, cfg, parts):
    """LoadToFITS over the stream cut into `parts`: (header values, blocks on the host, blocks completed by each call)"""
    lt = pipeline.LoadToFITS(cfg, pipeline.InputInfo(**SHAPES[name]["info"]), device=0, stream=torch.cuda.current_stream().cuda_stream)
    blocks, per_call = [], []
    for call in calls_of(name, parts):
        done = lt.process_block(torch.from_numpy(np.array(call[0])).cuda(), *call[1:])
        per_call.append(len(done))
        blocks.extend(tuple(t.cpu().numpy().copy() for t in blk) for blk in done)
    hv, tres, nblock, nblocks_out = lt.header_values(), lt.tres_factor, lt.nblock, lt.nblocks_out
    lt.synchronize()
    lt.close()
    assert nblocks_out == len(blocks)
    return hv, blocks, per_call, tres, nblock


_rows = {}


def reference_rows(dspsr_amd, pipeline, name, npol):
    """the scrunched rows [nchan][npol][N] of the whole stream from the front end's own, already-tested detect_scrunch (device)"""
    if (name, npol) in _rows:
        return _rows[name, npol]
    s = SHAPES[name]
    cls, kw = s["front"]
    scfg = pipeline.SearchConfig(**kw, nbit=8, rescale_seconds=0.0, npol=npol)
    lt = getattr(pipeline, cls)(scfg, pipeline.InputInfo(**s["info"]), device=0, stream=torch.cuda.current_stream().cuda_stream)
    got = [lt.detect_scrunch(torch.from_numpy(np.array(c[0])).cuda(), *c[1:]).clone() for c in calls_of(name, s["parts"][0])]
    lt.synchronize()
    assert abs(lt.out_rate - s["out_rate"]) <= 1e-9 * s["out_rate"]
    lt.close()
    _rows[name, npol] = torch.cat(got, dim=2).contiguous()
    return _rows[name, npol]


def by_hand(dspsr_amd, ctx, name, rows, npol, nbit, dedisperse, nblock, constant):
    """[SampleDelay at the scrunched rate] -> FITSDigitizer over every whole block of the rows, from the existing operators"""
    s = SHAPES[name]
    info = s["info"]
    nchan = rows.shape[0]
    if dedisperse:
        delays = dspsr_amd.dedispersion_sample_delays(info["centre_frequency"], info["bandwidth"], s["fits"]["dispersion_measure"], nchan,
                                                      s["out_rate"], **s["swap"])
        assert int(delays.max() - delays.min()) > 0
        sd = dspsr_amd.SampleDelay(ctx, delays, npol)
        out = torch.empty_like(rows)
        nd = sd.transform(rows, out)
        assert nd == rows.shape[2] - int(delays.max() - delays.min())
        rows = out[:, :, :nd]
        sd.close()
    dig = dspsr_amd.FITSDigitizer(ctx, nchan, npol, nbit, NSBLK, nblock, constant, flip_band=info["bandwidth"] > 0)
    blocks = []
    for k in range(rows.shape[2] // NSBLK):
        data = torch.empty(dig.block_bytes, dtype=torch.uint8, device="cuda")
        scl, offs = (torch.empty(nchan * npol, dtype=torch.float32, device="cuda") for _ in range(2))
        dig.pack(rows[:, :, k * NSBLK:(k + 1) * NSBLK], data, scl, offs)
        blocks.append((data.cpu().numpy(), scl.cpu().numpy(), offs.cpu().numpy()))
    dig.close()
    return blocks, rows.shape[2]


def same_blocks(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]), (what, k, "bytes")
        assert np.array_equal(x[1].view(np.int32), y[1].view(np.int32)) and np.array_equal(x[2].view(np.int32), y[2].view(np.int32)), (what, k, "scales")


@pytest.mark.parametrize("name,npol,nbit,dedisperse,extra", RUNS)
def test_load_to_fits_equals_the_operators_by_hand(gpu, tmp_path, name, npol, nbit, dedisperse, extra):
    dspsr_amd, ctx = gpu
    from dspsr_amd import pipeline
    s = SHAPES[name]
    cfg = fits_config(pipeline, name, npol, nbit, dedisperse, extra)
    hv, blocks, per_call, tres, nblock = run_fits(pipeline, name, cfg, s["parts"][0])
    assert tres == s["tres"] and hv["TBIN"] == 1.0 / s["out_rate"] and hv["NSBLK"] == NSBLK and hv["NPOL"] == npol and hv["NBITS"] == nbit
    # -I 0.004 with blocks of 128 x 16 us = 2.048 ms: unsigned(1.95 + 0.5) = 2; -I 0.0015 with 128 x 4 us (the REQUESTED tsamp): 3
    assert nblock == {0.004: 2, 0.0015: 3}.get(extra.get("rescale_seconds"), 1)
    want, nrows = by_hand(dspsr_amd, ctx, name, reference_rows(dspsr_amd, pipeline, name, npol), npol, nbit, dedisperse, nblock,
                          bool(extra.get("rescale_constant")))
    assert len(want) >= 5 and nrows % NSBLK, "the stream ends inside a block"        # the tail short of a block is absent
    same_blocks(blocks, want, "one call")
    lev = fc.unpack_levels(blocks[1][0], nbit)
    assert len(np.unique(lev)) > 1
    # the stream cut into unequal calls: a call that completes no block, one that completes at least three
    hv2, blocks2, per_call2, _, _ = run_fits(pipeline, name, cfg, s["parts"][1])
    assert 0 in per_call2 and max(per_call2) >= 3 and sum(per_call2) == len(want), per_call2
    assert hv2 == hv
    pipeline.write_search_blocks(tmp_path / "a.sblk", hv, blocks)
    pipeline.write_search_blocks(tmp_path / "b.sblk", hv2, blocks2)
    a, b = (tmp_path / "a.sblk").read_bytes(), (tmp_path / "b.sblk").read_bytes()
    assert a == b and len(a) == pipeline.SEARCH_BLOCKS_HDR_SIZE + len(want) * (8 * hv["NCHAN"] * npol + NSBLK * npol * hv["NCHAN"] * nbit // 8)
    # the file round-trips
    hdr, back = pipeline.read_search_blocks(tmp_path / "a.sblk")
    same_blocks(back, blocks, "read_search_blocks")
    assert int(hdr["NSBLK"]) == NSBLK and float(hdr["TBIN"]) == hv["TBIN"] and float(hdr["ZERO_OFF"]) == 2.0 ** (nbit - 1) - 0.5
    assert hdr["POL_TYPE"] == {1: "AA+BB", 2: "AABB", 4: "AABBCRCI"}[npol] and float(hdr["OBSBW"]) == -abs(s["info"]["bandwidth"])
    assert float(hdr["CHAN_BW"]) == -abs(s["info"]["bandwidth"]) / hv["NCHAN"] and int(hdr["NROWS"]) == len(want)


def test_tool_writes_the_pipelines_file(gpu, tmp_path, capsys):
    """tools/dspsr_amd_digifits.py on a DADA file, its own cut of the stream (5 parts per call): the file of the pipeline run above"""
    dspsr_amd, ctx = gpu
    from dspsr_amd import pipeline, synth
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dspsr_amd_digifits as tool
    s = SHAPES["real"]
    raw, _ = stream_of("real")
    i = s["info"]
    path = tmp_path / "real.dada"
    with open(path, "wb") as f:
        f.write(synth.dada_header(i["centre_frequency"], i["bandwidth"], 1, 2, 1, i["tsamp_us"], instrument="DADA", source="J0000+0000"))
        f.write(raw.tobytes())
    out = tmp_path / "real.sblk"
    assert tool.main([str(path), "-F", "16:D", "-x", "256", "-D", "1", "-do_dedisp", "true", "-t", "16e-6", "-p", "2", "-b", "4", "-nsblk", str(NSBLK),
                      "-I", "0.004", "-o", str(out), "--parts", "5"]) == 0
    err = capsys.readouterr().err
    assert "digifits: requested tsamp=1.6e-05 rate=3.2e+07" in err and "actual tsamp=1.6e-05 (tscrunch=16)" in err
    cfg = fits_config(pipeline, "real", 2, 4, False, dict(rescale_seconds=0.004))
    hv, blocks, _, _, _ = run_fits(pipeline, "real", cfg, s["parts"][0])
    hdr, got = pipeline.read_search_blocks(out)
    same_blocks(got, blocks, "tool")
    assert hdr["SRC_NAME"] == "J0000+0000" and int(hdr["STT_IMJD"]) == 55299 and float(hdr["TBIN"]) == hv["TBIN"]
    want = tmp_path / "want.sblk"
    pipeline.write_search_blocks(want, {**hv, "SRC_NAME": "J0000+0000", "STT_IMJD": int(hdr["STT_IMJD"]), "STT_SECONDS": float(hdr["STT_SECONDS"])}, blocks)
    assert want.read_bytes() == out.read_bytes()


def test_dispersed_pulse_arrives_where_the_dispersion_law_says(gpu):
    """A pulse-modulated noise signal dispersed with DM 100 over a 16 MHz band (dspsr_amd.synth: the cold-plasma transfer function of the
    whole band), digifits -F 16:D -D 100 -t 16e-6 -p 1 -b 8 -nsblk 128; the period is 128 output samples.  The decoded Intensity
    (level - ZERO_OFF) * DAT_SCL + DAT_OFFS folded at the period: with -do_dedisp true every channel peaks, sharply, in the sample its
    centre frequency's arrival time names (t = P/2 + D (1/nu^2 - 1/fc^2)); without, the pulse is smeared over 0.3 ms = 19 samples
    inside each channel and no such peak exists.
    "In the sample": the largest folded sample is the named one or a neighbour.  The envelope is a Gaussian of sigma 2.7 samples, so one
    sample off its top it has fallen by 1 / (2 * 2.7^2) = 6.8 % of the pulse height A = 3; a folded sample is a chi-square of
    64 degrees of freedom (16 complex samples, 2 polarisations) averaged over 40 periods at a level of 4: rms 4 * sqrt(2 / 2560) = 0.11
    = 3.7 % of A.  A neighbour outshines the top sample at 2 sigma, two samples off (27 %) never."""
    dspsr_amd, ctx = gpu
    from dspsr_amd import pipeline, synth
    freq, bw, tsamp_us, dm, nchan, tout, nbin = 1400.0, -16.0, 1.0 / 32.0, 100.0, 16, 16e-6, 128
    period = nbin * tout
    info = pipeline.InputInfo(centre_frequency=freq, bandwidth=bw, nchan=1, npol=2, ndim=1, tsamp_us=tsamp_us, machine="DADA")
    profiles = {}
    for coherent in (True, False):
        cfg = pipeline.FitsConfig(nchan=nchan, convolve=True, dispersion_measure=dm, coherent_dedisp=coherent, tsamp=tout, npol=1, nbit=8,
                                  nsblk=NSBLK, parts_per_block=8 if coherent else 4096)
        lt = pipeline.LoadToFITS(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
        front = lt.front
        assert (front.response.kernel is not None) == coherent and lt.tres_factor == 16
        nparts = -(-(40 * NSBLK * 16 * 32) // front.nsamp_step)                 # 40 blocks
        nparts += (-nparts) % cfg.parts_per_block
        ndat = nparts * front.nsamp_step + front.nsamp_overlap
        raw = synth.voltages(ndat, freq, bw, tsamp_us, dm, period, npol=2, ndim=1, pulse_amp=3.0)
        series = []
        for b in range(nparts // cfg.parts_per_block):
            s0 = b * cfg.parts_per_block * front.nsamp_step
            blk = raw[s0 * 2:(s0 + cfg.parts_per_block * front.nsamp_step + front.nsamp_overlap) * 2]
            for data, scl, offs in lt.process_block(torch.from_numpy(blk).cuda(), cfg.parts_per_block):
                lev = data.cpu().numpy().astype(np.float64).reshape(NSBLK, nchan)
                series.append((lev - 127.5) * scl.cpu().numpy().astype(np.float64) + offs.cpu().numpy().astype(np.float64))
        x = np.concatenate(series)                                               # [time][chan]
        assert x.shape[0] >= 30 * NSBLK
        t0, rate = lt.out_start, lt.out_rate
        lt.close()
        bins = np.floor(((t0 + (np.arange(x.shape[0]) + 0.5) / rate) / period % 1.0) * nbin).astype(int)
        prof = np.stack([np.bincount(bins, weights=x[:, c], minlength=nbin) / np.bincount(bins, minlength=nbin) for c in range(nchan)])
        profiles[coherent] = prof - prof.mean(axis=1, keepdims=True)
    peaked = {}
    for coherent, prof in profiles.items():
        flags = []
        for c in range(nchan):
            nu = freq - 0.5 * bw + (c + 0.5) * bw / nchan                        # output channel c (lower sideband: no flip)
            expected = ((0.5 * period + dm / DM_CONST * (1.0 / nu ** 2 - 1.0 / freq ** 2)) / period) % 1.0 * nbin
            d = (prof[c].argmax() - math.floor(expected) + nbin // 2) % nbin - nbin // 2
            sharp = prof[c].max() / prof[c].std()
            print("do_dedisp %s channel %2d: peak %3d expected %6.2f sharpness %.2f" % (coherent, c, prof[c].argmax(), expected, sharp))
            flags.append(abs(d) <= 1.0 and sharp >= 4.0)
        peaked[coherent] = flags
    assert all(peaked[True]) and not any(peaked[False])
