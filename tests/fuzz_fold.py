"""tests/fuzz_fold.py [ncases] [seed] : random fold shapes and bin plans against tests/fold_reference.py, bit for bit: the CPU
loop (Fold.C:835-891, strict time order) for the exact kernels, fold_long_model for plans that take the long-run fold (the
kernel fold_reference.fold_dispatch names); hits identical.  The rows sit at a random float offset with padded rows (NaN
around them), and some cases fold into a profile bound to a padded caller buffer.  Also random LoadToFold configurations,
fused against Detection + Fold, and -- where the fold of every block is one call of the fused kernels (fold_is_fused() 1 or 2) --
against fold_reference.fused_fold_model bit for bit; each configuration also with the library's own choice (FUSED_AUTO), which is
where the segmented launches (mode 2) come from."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dspsr_amd
from dspsr_amd import pipeline, synth
from device_buffers import device_rows
from fused_fold_cases import FOLD_FUSED_MAX_RUN, loadtofold_block_model
from fold_reference import fold_dispatch, fold_long_model, fold_time_order, runs_of_plan

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
ncu = torch.cuda.get_device_properties(0).multi_processor_count


ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
bad = 0
for i in range(ncases):
    ndim = int(rng.choice([1, 2, 4]))
    npol = 4 // ndim if rng.integers(0, 3) else 1
    nchan = int(rng.choice([1, 3, 17, 64, 300, 700]))
    nbin = int(rng.choice([8, 31, 64, 100, 500, 1024, 2048, 5000]))
    ndat = int(rng.integers(50, 40000))
    spb = float(rng.choice([0.3, 1.7, 9.0, 40.0, 90.0, 700.0, 5000.0]))          # samples per bin
    pps = 1.0 / (spb * nbin)
    phi = float(rng.random())
    idat_start = int(rng.integers(0, 40))
    ndat_fold = ndat - idat_start - int(rng.integers(0, 10))
    det = (rng.standard_normal((nchan, npol, ndat, ndim)).astype(np.float32)) ** 2
    # placement: a second generator seeded with (seed, case), so that the draws above -- the geometry of a seed -- stay as they were
    r2 = np.random.default_rng((seed, i))
    # (half the cases keep the allocator's alignment: shifted rows all take k_fold_direct)
    offset, row_pad = int(r2.choice([0, 0, 0, 1, 2, 3])), int(r2.choice([0, 0, 0, 1, 3, 4]))
    bound = bool(r2.integers(0, 3) == 0)
    d = device_rows(det.reshape(nchan, npol, ndat * ndim), offset, row_pad)
    eng = dspsr_amd.FoldEngine(ctx)
    if bound:                                                    # a caller's profile: padded rows at an odd float offset, NaN padding
        span = nbin * ndim + int(r2.integers(1, 5))
        pbuf = torch.full((64 + 1 + nchan * npol * span,), float("nan"), dtype=torch.float32, device="cuda")
        prof = pbuf[1:1 + nchan * npol * span].view(nchan * npol, span)
        prof[:, :nbin * ndim] = 0.0
        eng.bind_profile(prof, nchan, npol, ndim, nbin)
    else:
        eng.set_shape(nchan, npol, ndim, nbin)
    hits = np.zeros(nbin, np.uint32)
    eng.set_nbin(nbin)
    eng.set_ndat(ndat_fold, idat_start)
    eng.set_bins(phi, pps, ndat_fold, idat_start, hits)
    eng.fold(d)
    got = eng.synch()
    pad_ok = True
    if bound:
        pad_ok = bool(torch.isnan(prof[:, nbin * ndim:]).all()) and bool(torch.isnan(pbuf[:1]).all())
    eng.close()
    plan, want_hits = dspsr_amd.fold_binplan(phi, pps, nbin, ndat_fold)
    runs = runs_of_plan(plan, idat_start)
    kernel = fold_dispatch(d.data_ptr(), d.stride(0), d.stride(1), nchan, npol, ndim, nbin, runs, ncu)["kernel"]
    zero = np.zeros((nchan, npol, nbin, ndim), np.float32)
    want = fold_long_model(det, runs, zero, nchan * npol, ncu) if kernel == "long" else fold_time_order(det, runs, zero)
    desc = "nchan=%d npol=%d ndim=%d nbin=%d ndat=%d samples/bin=%g offset=%d row_pad=%d%s -> %s" % (
        nchan, npol, ndim, nbin, ndat_fold, spb, offset, row_pad, " bound" if bound else "", kernel)
    ok_hits = np.array_equal(hits, want_hits)
    exact = np.array_equal(got, want)
    if ok_hits and exact and pad_ok:
        print("ok   ", desc, flush=True)
    else:
        bad += 1
        print("FAIL ", desc, "hits", ok_hits, "exact", exact, "padding", pad_ok, flush=True)
# pipeline: fused against separate launches
for i in range(max(4, ncases // 3)):
    freq = float(rng.choice([1382.0, 400.0, 3100.0]))
    bw = float(rng.choice([-16.0, 16.0, -64.0, 8.0]))
    tsamp = 1.0 / (2.0 * abs(bw))                      # real sampling of the band
    dm = float(rng.choice([0.0, 3.0, 30.0, 120.0]))
    nchan = int(2 ** rng.integers(1, 10))
    nbin = int(rng.choice([16, 64, 256, 1024]))
    period = float(rng.choice([0.0007, 0.004, 0.0371]))
    ppb, mp = int(rng.integers(1, 6)), int(rng.integers(1, 4))
    sub = float(rng.choice([0.0, 0.0, 0.0021]))
    info = pipeline.InputInfo(centre_frequency=freq, bandwidth=bw, tsamp_us=tsamp, machine="DADA")
    res, modes, exact, modelled = [], [], [], []
    refused = None
    for fused, forced in ((True, True), (False, False), (True, False)):
        cfg = pipeline.Config(nchan=nchan, dispersion_measure=dm, nbin=nbin, folding_period=period, ndim=4, parts_per_block=ppb,
                              max_parts=mp, fused_fold=fused, force_fused=forced, subint_seconds=sub)
        try:
            lt = pipeline.LoadToFold(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
            if 3 * ppb * lt.nsamp_step + lt.nsamp_overlap > (1 << 25):
                lt.close()
                raise dspsr_amd.DspsrAmdError("block too long for a sweep")
        except dspsr_amd.DspsrAmdError as e:
            refused = str(e)
            break
        step = ppb * lt.nsamp_step
        raw = torch.from_numpy(synth.voltages(3 * step + lt.nsamp_overlap, freq, bw, tsamp, max(dm, 1.0), period, seed=7 + i)).cuda()
        # the model: one sub-integration, every block folded by one call of the fused kernels (None as soon as one is not)
        model = np.zeros((nchan, 1, nbin, 4), np.float32) if sub == 0.0 and lt.fused_mode in (1, 2) else None
        for b in range(3):
            block = raw[2 * b * step: 2 * (b * step + step + lt.nsamp_overlap)]
            if model is not None:
                table_mode, _h, model = loadtofold_block_model(lt, block, ppb, model, ncu)
                if model is None:
                    print("note  block %d of the %s run has a run of %d samples or more: Detection + Fold there, no exact model for this run"
                          % (b, "forced" if forced else "auto", FOLD_FUSED_MAX_RUN), flush=True)
                if table_mode != lt.fused_mode:
                    bad += 1
                    print("FAIL  fold_is_fused() %d, the table says %d" % (lt.fused_mode, table_mode), flush=True)
            lt.process_block(block)
        if lt.ndat_total:
            lt.finish_subint()
        lt.synchronize()
        res.append([(s["hits"].copy(), s["profile_dev"].cpu().numpy(), s["ndat_total"]) for s in lt.subints])
        modes.append(lt.fused_mode)
        modelled.append(model is not None)
        exact.append(model is None or (len(res[-1]) == 1 and np.array_equal(res[-1][0][1].reshape(-1), model.reshape(-1))))
        freq_res = lt.response.ndat
        lt.close()
    if refused is not None:
        print("refused pipeline freq=%g bw=%g DM=%g nchan=%d -- %s" % (freq, bw, dm, nchan, refused[:90]), flush=True)
        continue
    desc = "pipeline freq=%g bw=%g DM=%g nchan=%d freq_res=%d nbin=%d period=%g parts/block=%d max_parts=%d subint=%g (%d sub-integrations, mode %d, auto %d)" % (
        freq, bw, dm, nchan, freq_res, nbin, period, ppb, mp, sub, len(res[0]), modes[0], modes[2])
    desc += " exact model: %s" % "/".join("yes" if m else "-" for m in (modelled[0], modelled[2]))
    good = len(res[0]) == len(res[1]) == len(res[2]) and all(exact)
    for a, b in list(zip(res[0], res[1])) + list(zip(res[2], res[1])):
        # (float32 sums of N samples per bin, associated differently by the two paths: the same sqrt(N) allowance as above --
        #  186 000 hits per bin gave 3.8e-6, identical for every launch shape)
        scale = max(np.abs(b[1]).max(), 1e-30) * max(1.0, (float(b[0].max()) / 100.0) ** 0.5)
        good = good and np.array_equal(a[0], b[0]) and a[2] == b[2] and np.abs(a[1] - b[1]).max() <= 2e-6 * scale
    if good:
        print("ok   ", desc, flush=True)
    else:
        bad += 1
        print("FAIL ", desc, flush=True)
ctx.close()
print("%d failures" % bad)
sys.exit(1 if bad else 0)
