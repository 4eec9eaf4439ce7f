"""SIGPROC filterbank files through dada.fold_file: small files written with write_sigproc_header, folded by the detected back end
(pipeline.DetectedFold) and compared BIT FOR BIT with a float64 fold of the restatement's rows (tests/sigproc_cases.py).

The inputs are small integers (and half-integers where the unpacker takes 127.5 off), so every (channel, polarisation, bin) total
of magnitudes stays below 2^23 -- asserted on the host for every case -- and is a multiple of 0.5: float32 sums are then exact in
any order, and the device's profile must EQUAL the float64 index_add by fold_binplan, with hits and integration length equal."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import sigproc_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = sc.ROOT
NCHAN, NDAT, BLOCK, NBIN, PERIOD = 64, 20000, 4096, 64, 0.0101


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    return dspsr_amd


def _values(nbit, nchan, npol, ndat, top, seed=0):
    """integers 0 ... top [ndat][npol][nchan] with a pulse of period PERIOD in them"""
    rng = np.random.default_rng(100 * nbit + npol + seed)
    v = rng.integers(0, top // 2 + 1, (ndat, npol, nchan))
    t = np.arange(ndat) * sc.HEADER["tsamp"]
    on = ((t / PERIOD) % 1.0) < 0.1
    v[on] += top - top // 2
    return v


def _block_counts(ndat, block, head=0):
    """output samples of every block: -K gives up `head` samples at the end of a block and carries them (DelayCarry)"""
    counts, carried = [], 0
    for b in range(0, ndat, block):
        n = min(block, ndat - b)
        nout = max(carried + n - head, 0)
        counts.append(nout)
        carried = carried + n - nout
    return counts


def host_fold(dspsr_amd, rows, rate, out_start, counts, periods_nbins, L=0.0):
    """The fold of rows float32 [nchan][npol][N] in float64, block by block and piece by piece as Subint<Fold> cuts them: the
    phase of a piece's first sample (Fold.C:650-657), fold_binplan's bins, index_add.  Returns per pulsar the list of
    (hits, integration_length, ndat_total, profile float64 [nchan][npol][nbin]) of its sub-integrations; asserts the bound that
    makes float32 sums exact."""
    from dspsr_amd import pipeline
    x = torch.from_numpy(rows.astype(np.float64))
    out = []
    for period, nbin in periods_nbins:
        prof, mag = torch.zeros(x.shape[:2] + (nbin,), dtype=torch.float64), torch.zeros(x.shape[:2] + (nbin,), dtype=torch.float64)
        hits, length, total, subs, pos = np.zeros(nbin, np.uint32), 0.0, 0, [], 0
        for n in counts:
            for i0, m, _k, done in (pipeline.subint_pieces(pos, n, L, rate) if L else [(0, n, 0, False)] if n else []):
                t0 = out_start + (pos + i0 + 0.5) / rate
                plan, h = dspsr_amd.fold_binplan(math.fmod(t0, period) / period, (1.0 / rate) / period, nbin, m)
                idx = torch.from_numpy(plan.astype(np.int64))
                prof.index_add_(2, idx, x[:, :, pos + i0:pos + i0 + m])
                mag.index_add_(2, idx, x[:, :, pos + i0:pos + i0 + m].abs())
                hits += h
                length += m / rate
                total += m
                if done:
                    subs.append((hits.copy(), length, total, prof.numpy().copy()))
                    prof.zero_()
                    hits[:] = 0
                    length, total = 0.0, 0
            pos += n
        if total:
            subs.append((hits.copy(), length, total, prof.numpy().copy()))
        assert float(mag.max()) < 2.0 ** 23 and pos <= rows.shape[2], "the case leaves the range where float32 sums are exact"
        assert np.array_equal(np.asarray([s[3] for s in subs]) * 2, np.rint(np.asarray([s[3] for s in subs]) * 2))
        out.append(subs)
    return out


def _compare(got_subints, want, nchan, npol, nbin, what):
    assert len(got_subints) == len(want), "%s: %d sub-integrations, %d expected" % (what, len(got_subints), len(want))
    for k, (sub, (hits, length, total, prof)) in enumerate(zip(got_subints, want)):
        got = sub["profile_dev"].cpu().numpy().reshape(nchan, npol, nbin).astype(np.float64)
        assert np.array_equal(sub["hits"], hits), "%s: hits of sub-integration %d" % (what, k)
        assert sub["ndat_total"] == total and sub["integration_length"] == length, "%s: books of sub-integration %d" % (what, k)
        bad = np.argwhere(got != prof)
        assert bad.size == 0, "%s: sub-integration %d: %d sums differ, the first (chan, pol, bin) %s: %r, expected %r" % (
            what, k, len(bad), tuple(bad[0]), got[tuple(bad[0])], prof[tuple(bad[0])])
        assert np.abs(prof).max() > 0


def _fold_file(path, nchan, nbin=NBIN, block=BLOCK, **kw):
    from dspsr_amd import dada, pipeline
    cfg = pipeline.Config(**dict(dict(nchan=nchan, nbin=nbin, folding_period=PERIOD, parts_per_block=block), **kw))
    return dada.fold_file(path, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)


def _case(tmp_path, nbit, npol, top, name, nchan=NCHAN, ndat=NDAT):
    v = _values(nbit, nchan, npol, ndat, top)
    if nbit == 16 and npol == 4:
        v[:, 2:] += 32768 - top // 2           # the cross products lie around the 32768 the unpacker takes off: small magnitudes
    raw = sc.pack(v.astype(np.float32) if nbit == 32 else v, nbit)
    path = str(tmp_path / name)
    sc.write_fil(path, raw, nbits=nbit, nchans=nchan, nifs=npol)
    return path, sc.unpack_fpt(raw, nbit, nchan, npol, ndat)


# (a) nbit 8, (c) nifs 4 with the 127.5 of products 2 and 3, (d) nbit 2, (e) nbit 32 as floats; nbit 16 below 4096; 1 and 4 bits; PPQQ
@pytest.mark.parametrize("nbit,npol,top", [(8, 1, 255), (8, 4, 255), (2, 1, 3), (32, 1, 1000), (16, 2, 4095), (1, 1, 1), (4, 2, 15), (16, 4, 4095)])
def test_fold_file_of_a_filterbank_file(gpu, tmp_path, nbit, npol, top):
    """20 000 spectra of 64 channels in blocks of 4096: five blocks, the last ragged"""
    path, rows = _case(tmp_path, nbit, npol, top, "a.fil")
    if nbit in (8, 16) and npol == 4:
        assert rows[:, 2:].min() < 0 and rows[:, :2].min() >= 0                     # the offset of the cross products is in the case
    lt = _fold_file(path, NCHAN)
    try:
        from dspsr_amd import pipeline
        assert isinstance(lt.mode, pipeline.DetectedFold) and lt.fb is None and lt.state_name() == {1: "Intensity", 2: "PPQQ", 4: "Coherence"}[npol]
        assert lt.ndat_out == lt.nsamples_in == NDAT and (lt.nchan_out, lt.npol_out) == (NCHAN, npol)
        want = host_fold(gpu, rows, lt.out_rate, lt.out_start, _block_counts(NDAT, BLOCK), [(PERIOD, NBIN)])[0]
        _compare(lt.subints, want, NCHAN, npol, NBIN, "nbit %d npol %d" % (nbit, npol))
    finally:
        lt.close()


def test_interchannel_delays(gpu, tmp_path):
    """(b) -K at a DM whose largest delay is a few hundred samples: more than zero, less than a block -- the carry is used on every
    block and the tail falls off.  Against the restatement's rows delayed in numpy (SampleDelay.C:123-195)."""
    path, rows = _case(tmp_path, 8, 1, 255, "k.fil")
    dm = 240.0
    lt = _fold_file(path, NCHAN, interchan_dedispersion=True, dispersion_measure=dm, record_time=True)
    try:
        d = gpu.dedispersion_sample_delays(lt.info.centre_frequency, lt.info.bandwidth, dm, NCHAN, lt.info.rate)
        zero, head = int(d.max()), int((d.max() - d).max())
        assert 100 < head < 1000 and (lt.sd.head, lt.sd.zero, lt.sd.carried) == (head, zero, head)
        assert lt.out_start == zero / lt.out_rate and lt.ndat_out == NDAT - head
        delayed = np.stack([rows[c, :, zero - d[c]:zero - d[c] + NDAT - head] for c in range(NCHAN)])
        want = host_fold(gpu, delayed, lt.out_rate, lt.out_start, _block_counts(NDAT, BLOCK, head), [(PERIOD, NBIN)])[0]
        _compare(lt.subints, want, NCHAN, 1, NBIN, "-K")
        assert list(lt.optime) == ["SigProcUnpacker", "SampleDelay", "Fold"] and lt.optime["Fold"][1] == 5
    finally:
        lt.close()


def test_sub_integrations(gpu, tmp_path):
    """(f) -L of 6144 samples: the boundary at 6144 lies inside the second block, the one at 12288 exactly on the end of the third,
    the one at 18432 inside the last"""
    path, rows = _case(tmp_path, 8, 2, 255, "l.fil")
    L = 6144 * sc.HEADER["tsamp"]
    lt = _fold_file(path, NCHAN, subint_seconds=L)
    try:
        want = host_fold(gpu, rows, lt.out_rate, lt.out_start, _block_counts(NDAT, BLOCK), [(PERIOD, NBIN)], L=L)[0]
        assert [w[2] for w in want] == [6144, 6144, 6144, NDAT - 3 * 6144]
        _compare(lt.subints, want, NCHAN, 2, NBIN, "-L")
    finally:
        lt.close()


def test_two_targets_fold_in_one_shared_launch(gpu, tmp_path, monkeypatch):
    """(g) two pulsars over the same rows: FoldEngine.fold_many takes both in a shared launch on every block"""
    from dspsr_amd import pipeline
    path, rows = _case(tmp_path, 8, 1, 255, "g.fil")
    shared, fold_many = [], gpu.FoldEngine.fold_many
    monkeypatch.setattr(gpu.FoldEngine, "fold_many", staticmethod(lambda folds, inp: shared.append(fold_many(folds, inp)) or shared[-1]))
    targets = [pipeline.FoldTarget(name="a", folding_period=PERIOD, nbin=NBIN), pipeline.FoldTarget(name="b", folding_period=0.0037, nbin=32)]
    from dspsr_amd import dada
    cfg = pipeline.Config(nchan=NCHAN, nbin=NBIN, parts_per_block=BLOCK)
    lt = dada.fold_file(path, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream, targets=targets)
    try:
        assert shared == [2] * 5 and len(lt.pulsars) == 2
        want = host_fold(gpu, rows, lt.out_rate, lt.out_start, _block_counts(NDAT, BLOCK), [(PERIOD, NBIN), (0.0037, 32)])
        for p, w, nbin in zip(lt.pulsars, want, (NBIN, 32)):
            _compare(p.subints, w, NCHAN, 1, nbin, "pulsar %s" % p.target.name)
    finally:
        lt.close()


def test_round_trip_through_the_search_driver(gpu, tmp_path):
    """(h) LoadToFil writes an 8-bit file from a short synthetic voltage block at its smallest geometry (16 channels, tscrunch 4);
    fold_file folds that file: the restatement on the bytes LoadToFil wrote"""
    from dspsr_amd import pipeline, sigproc
    nchan, tscr, npart, nblocks = 16, 4, 512, 3
    info = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=-400.0, tsamp_us=0.00125, machine="DADA", source="J0437-4715")
    scfg = pipeline.SearchConfig(nchan=nchan, tscrunch=tscr, nbit=8, rescale_seconds=(npart // tscr + 0.5) * 2 * nchan * tscr * 0.00125e-6, parts_per_block=npart)
    lf = pipeline.LoadToFil(scfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
    rng, packed = np.random.default_rng(8), []
    try:
        for b in range(nblocks):
            raw = np.clip(np.rint(rng.standard_normal(npart * 2 * nchan * 2) * (20.0 + 6 * b)), -128, 127).astype(np.int8)
            packed.append(lf.process_block(torch.from_numpy(raw).cuda()).cpu().numpy().copy())
        lf.synchronize()
        header = lf.header_values()
    finally:
        lf.close()
    data = np.concatenate(packed)
    ndat = nblocks * npart // tscr
    assert data.size == ndat * nchan and len(np.unique(data)) > 32
    path = str(tmp_path / "h.fil")
    with open(path, "wb") as f:
        pipeline.write_sigproc_header(f, source_name=info.source, rawdatafile="h.dada", **header)
        f.write(data.tobytes())
    sf = sigproc.SigprocFile(path)
    assert (sf.ndat, sf.info.nchan, sf.info.npol, sf.info.nbit, sf.info.detected) == (ndat, nchan, 1, 8, "Intensity")
    assert sf.info.rate == pytest.approx(1.0 / header["tsamp"], rel=1e-15) and sf.info.bandwidth == -400.0 and sf.info.centre_frequency == pytest.approx(1382.0, abs=1e-9)
    rows = sc.unpack_fpt(data, 8, nchan, 1, ndat)
    period, nbin, block = 37.3 / sf.info.rate, 16, 100
    lt = _fold_file(path, nchan, nbin=nbin, block=block, folding_period=period)
    try:
        want = host_fold(gpu, rows, lt.out_rate, lt.out_start, _block_counts(ndat, block), [(period, nbin)])[0]
        _compare(lt.subints, want, nchan, 1, nbin, "round trip")
    finally:
        lt.close()


def test_fold_tool_takes_the_file_with_no_filterbank_option(gpu, tmp_path):
    """tools/dspsr_amd_fold.py -K -D ... -c ... file.fil as a fresh child process: PhaseSeries files whose STATE / NPOL / NCHAN are
    the file's, the sums those of the pipeline call"""
    from dspsr_amd import pipeline
    path, rows = _case(tmp_path, 8, 2, 255, "t.fil", ndat=6000)
    prefix = str(tmp_path / "tool")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dspsr_amd_fold.py"), "-K", "-D", "240", "-c", str(PERIOD), "-b", str(NBIN),
                        "-O", prefix, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    h, hits, prof = pipeline.read_phase_series(prefix + "_0000.ps")
    assert (h["STATE"], int(h["NPOL"]), int(h["NCHAN"]), int(h["NDIM"]), int(h["NBIN"])) == ("PPQQ", 2, NCHAN, 1, NBIN)
    lt = _fold_file(path, NCHAN, block=6000, interchan_dedispersion=True, dispersion_measure=240.0)
    try:
        assert int(h["NDAT_TOTAL"]) == hits.sum() == lt.subints[0]["ndat_total"] == 6000 - lt.sd.head
        assert np.array_equal(prof.reshape(-1), lt.subints[0]["profile_dev"].cpu().numpy().reshape(-1))
    finally:
        lt.close()
