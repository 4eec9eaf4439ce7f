"""Several pulsars from one detected stream: dspsr_amd_fold_fold_many (csrc/fold.hip k_fold_many) and the multi-target LoadToFold.

fold_many folds the exact-order plans of a call in shared launches that read the rows once, and the others (LONG runs, unaligned
rows) one by one.  Every profile must be bit-identical to fold_reference (fold_time_order; LONG: fold_long_model) and to
dspsr_amd_fold_fold of the same plan on a second engine, hits identical, and nshared the number of exact-order plans (0 when
there is only one: it is folded alone).  Sets larger than FOLD_MANY_MAX split into balanced launches.  The
multi-target LoadToFold must give each pulsar exactly the sub-integrations of a single-pulsar LoadToFold of that pulsar.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from fold_reference import fold_dispatch, fold_long_model, fold_many_dispatch, fold_time_order, runs_of_plan
from device_buffers import device_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx, torch.cuda.get_device_properties(0).multi_processor_count
    ctx.close()


# plan kinds: (samples per period, nbin).  dense: a period above FOLD_CHUNK, runs < 64; walk: periods below FOLD_CHUNK (several runs
# of a bin per chunk, the millisecond-pulsar case); long: runs >= FOLD_LONG_RUN (single-fold LONG path); weighted: a walk plan
# with zero-weight gaps; empty: set_nbin only
KINDS = ["dense", "walk", "long", "weighted", "empty", "walk_big", "dense_big", "walk_small"]
EXACT = [k for k in KINDS if k not in ("long", "empty")]          # the kinds that take a shared launch
SHAPE = {"dense": (4100.3, 128), "walk": (700.7, 32), "long": (20000.9, 64), "weighted": (900.3, 64), "empty": (1000.0, 16),
         "walk_big": (1500.1, 1024), "dense_big": (9000.5, 4096), "walk_small": (333.3, 8)}


def _plan(eng, oracle, kind, nbin, period, idat_start, n, seed):
    """hand the same plan to `eng`; returns (runs, hits)"""
    eng.set_nbin(nbin)
    eng.set_ndat(n, idat_start)
    hits = np.zeros(nbin, np.uint32)
    if kind == "empty":
        return np.zeros((0, 3), np.int64), hits
    rng = np.random.default_rng(seed)
    phi, pps = float(rng.random()), 1.0 / period
    plan = oracle.fold_binplan(phi, pps, nbin, n)
    if kind != "weighted":
        assert eng.set_bins(phi, pps, n, idat_start, hits) == n
        return runs_of_plan(plan, idat_start), hits
    ndpw = 64
    w = (rng.random((idat_start + n) // ndpw + 1) > 0.3).astype(np.uint32)
    eng.set_bins(phi, pps, n, idat_start, hits, weights=w, ndatperweight=ndpw)
    keep = w[(idat_start + np.arange(n)) // ndpw] != 0
    runs, s = [], 0
    while s < n:                                        # a dropped sample ends a run
        if not keep[s]:
            s += 1
            continue
        e = s
        while e < n and keep[e]:
            e += 1
        runs.append(runs_of_plan(plan[s:e], idat_start + s))
        s = e
    return np.concatenate(runs), hits


def _case(gpu, oracle, kinds, nchan, npol, ndim, ndat, offset=0, row_pad=0, rounds=2):
    dspsr_amd, ctx, ncu = gpu
    rng = np.random.default_rng(len(kinds) * 100 + ndim * 10 + npol)
    x = (rng.standard_normal((nchan, npol, ndat, ndim)) ** 2 + rng.random((nchan, npol, ndat, ndim))).astype(np.float32)
    d = device_rows(x.reshape(nchan, npol, ndat * ndim), offset, row_pad)
    many, single, want = [], [], []
    for kind in kinds:
        period, nbin = SHAPE[kind]
        for lst in (many, single):
            e = dspsr_amd.FoldEngine(ctx)
            e.set_shape(nchan, npol, ndim, nbin)
            lst.append(e)
        want.append(np.zeros((nchan, npol, nbin, ndim), np.float32))
    for rnd in range(rounds):                          # the second round folds into profiles that hold sums
        nexact = 0
        for k, kind in enumerate(kinds):
            period, nbin = SHAPE[kind]
            i0 = (37 * k + 11 * rnd) % 300             # every plan its own span
            n = ndat - i0 - (53 * k) % 400
            runs, h1 = _plan(many[k], oracle, kind, nbin, period, i0, n, seed=1000 * rnd + k)
            _, h2 = _plan(single[k], oracle, kind, nbin, period, i0, n, seed=1000 * rnd + k)
            assert np.array_equal(h1, h2) and np.array_equal(h1, np.bincount(runs[:, 1], weights=runs[:, 2], minlength=nbin).astype(np.uint32))
            if not len(runs):
                continue
            disp = fold_dispatch(d.data_ptr(), d.stride(0), d.stride(1), nchan, npol, ndim, nbin, runs, ncu)
            assert kind != "long" or disp["kernel"] == "long" or offset or row_pad % 4
            nexact += disp["kernel"] in ("dense", "chunked")
            want[k] = (fold_long_model(x, runs, want[k], nchan * npol, ncu) if disp["kernel"] == "long"
                       else fold_time_order(x, runs, want[k]))
        nshared = dspsr_amd.FoldEngine.fold_many(many, d)
        for e in single:
            e.fold(d)
        assert nshared == (nexact if nexact > 1 else 0)     # a lone exact-order plan is folded alone
    for k, kind in enumerate(kinds):
        got_many, got_single = many[k].synch(), single[k].synch()
        assert np.isfinite(got_many).all()
        assert np.array_equal(got_many, want[k]), kind
        assert np.array_equal(got_single, want[k]), kind
    for e in many + single:
        e.close()


@pytest.mark.parametrize("kinds,nchan,npol,ndim,ndat,offset,row_pad", [
    (KINDS[:2], 6, 1, 4, 9000, 0, 0),
    (KINDS[:3], 5, 2, 2, 9000, 0, 8),                     # padded rows
    (KINDS[:3], 4, 4, 1, 8000, 0, 0),
    (KINDS, 3, 1, 4, 12000, 0, 0),                        # every kind in one call: 6 shared, LONG and empty alone
    (KINDS, 4, 2, 2, 9000, 0, 4),
    (KINDS, 3, 4, 1, 9000, 0, 0),
    ((EXACT * 2)[:8], 3, 1, 4, 9000, 0, 0),               # a full launch: FOLD_MANY_MAX exact-order plans
    ((EXACT * 2)[:8], 3, 2, 2, 9000, 0, 0),
    ((EXACT * 2)[:9], 4, 1, 4, 9000, 0, 0),               # FOLD_MANY_MAX + 1 exact-order plans: two launches (5 + 4)
    ((EXACT * 3)[:17], 2, 4, 1, 6000, 0, 0),              # three launches (6 + 6 + 5)
    (["dense", "long", "empty"], 3, 1, 4, 7000, 0, 0),    # one exact-order plan: folded alone, nshared 0
    (KINDS[:3], 4, 2, 2, 7000, 1, 0),                     # rows off a 16-byte boundary: every plan folded alone
    (KINDS[:3], 3, 1, 4, 7000, 0, 3),                     # strides off the 4-float grid
])
def test_fold_many_bit_identical(gpu, oracle, kinds, nchan, npol, ndim, ndat, offset, row_pad):
    _case(gpu, oracle, list(kinds), nchan, npol, ndim, ndat, offset, row_pad)


@pytest.mark.parametrize("npol,ndim", [(2, 2), (4, 1)])
def test_fold_many_rows_per_workgroup(gpu, oracle, npol, ndim):
    """NROW > 1: enough channels that a workgroup folds all polarisation rows of its channel"""
    kinds = ["dense", "walk", "walk_small"]
    assert fold_many_dispatch(520, npol, ndim, sum(SHAPE[k][1] for k in kinds), gpu[2])["nrow"] == npol
    _case(gpu, oracle, kinds, 520, npol, ndim, 4500, rounds=1)


def test_fold_many_refusals_leave_plans(gpu, oracle):
    dspsr_amd, ctx, _ = gpu
    from dspsr_amd import _lib
    nchan, npol, ndim, ndat = 3, 1, 4, 6000
    rng = np.random.default_rng(5)
    x = rng.random((nchan, npol, ndat, ndim)).astype(np.float32)
    d = device_rows(x.reshape(nchan, npol, ndat * ndim), 0, 0)
    engs, runs = [], []
    for kind in ("dense", "walk"):
        period, nbin = SHAPE[kind]
        e = dspsr_amd.FoldEngine(ctx)
        e.set_shape(nchan, npol, ndim, nbin)
        runs.append(_plan(e, oracle, kind, nbin, period, 3, ndat - 10, seed=9)[0])
        engs.append(e)
    other = dspsr_amd.FoldEngine(ctx)
    other.set_shape(nchan + 1, npol, ndim, 32)
    _plan(other, oracle, "walk", 32, 700.7, 0, 100, seed=1)
    ctx2 = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    far = dspsr_amd.FoldEngine(ctx2)
    far.set_shape(nchan, npol, ndim, 32)
    _plan(far, oracle, "walk", 32, 700.7, 0, 100, seed=1)

    def call(handles):
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        return _lib.lib.dspsr_amd_fold_fold_many(arr, len(handles), d.data_ptr(), d.stride(0), d.stride(1), None)
    a, b = engs
    assert call([a.handle, a.handle]) == _lib.EINVAL
    assert call([a.handle, None]) == _lib.EINVAL
    assert call([a.handle, other.handle]) == _lib.EINVAL
    assert call([a.handle, far.handle]) == _lib.EINVAL
    assert call([]) == _lib.OK
    with pytest.raises(dspsr_amd.DspsrAmdError):
        dspsr_amd.FoldEngine.fold_many([b, a, b], d)
    assert dspsr_amd.FoldEngine.fold_many([a, b], d) == 2
    for e, r in zip(engs, runs):
        assert np.array_equal(e.synch(), fold_time_order(x, r, np.zeros((nchan, npol, e.synch().shape[2], ndim), np.float32)))
    for e in engs + [other, far]:
        e.close()
    ctx2.close()


# ---- the multi-target LoadToFold against one single-target LoadToFold per pulsar ------------------------------------------------

def _polyco():
    from dspsr_amd import pipeline
    return pipeline.Polyco(json.load(open(os.path.join(ROOT, "tests", "golden", "vela_polyco.json")))["text"])


def _run_lt(cfg, info, raw, nblocks, targets):
    from dspsr_amd import pipeline
    lt = pipeline.LoadToFold(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream, targets=targets)
    step = cfg.parts_per_block * lt.nsamp_step
    for b in range(nblocks):
        lt.process_block(raw[2 * b * step: 2 * (b * step + step + lt.nsamp_overlap)])
    if lt.ndat_total or lt.pulsars:
        lt.finish_subint()
    lt.synchronize()
    lists = [p.subints for p in lt.pulsars] if lt.pulsars else [lt.subints]
    out = [[(s["hits"].copy(), s["integration_length"], s["ndat_total"], s["profile_dev"].cpu().numpy()) for s in subs]
           for subs in lists]
    lt.close()
    return out


def _compare(multi, single):
    assert len(multi) == len(single) and len(multi) >= 1
    for m, s in zip(multi, single):
        assert np.array_equal(m[0], s[0]) and m[1] == s[1] and m[2] == s[2]
        assert np.isfinite(m[3]).all() and np.array_equal(m[3], s[3])


@pytest.mark.parametrize("name,ntarget,extra", [
    ("constant-2", 2, {}),
    ("polyco-3", 3, {}),
    ("L", 3, dict(subint_seconds=0.0031)),
    ("s", 2, dict(subint_turns=1.0)),
    ("after", 3, dict(convolve_when="after")),
    ("K", 3, dict(interchan_dedispersion=True)),
])
def test_load_to_fold_targets_match_single_pulsar_runs(gpu, name, ntarget, extra):
    from dspsr_amd import pipeline, synth
    freq, bw, tsamp, dm, nchan = 1382.0, -16.0, 1.0 / 32.0, 30.0, 16
    cfg = pipeline.Config(nchan=nchan, dispersion_measure=dm, nbin=64, ndim=4, parts_per_block=3, max_parts=2, **extra)
    info = pipeline.InputInfo(centre_frequency=freq, bandwidth=bw, tsamp_us=tsamp)
    targets = [pipeline.FoldTarget("a", folding_period=0.004, nbin=64),              # 4000 samples per period: dense
               pipeline.FoldTarget("b", folding_period=0.00123, nbin=32, reference_phase=0.25)]   # 1230: walk
    if ntarget == 3:
        targets.append(pipeline.FoldTarget("vela", polyco=_polyco()) if name != "s" else
                       pipeline.FoldTarget("c", folding_period=0.0021, nbin=16))
    probe = pipeline.LoadToFold(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream, targets=targets[:1])
    nblocks, step, overlap = 3, cfg.parts_per_block * probe.nsamp_step, probe.nsamp_overlap
    probe.close()
    raw = torch.from_numpy(synth.voltages(nblocks * step + overlap, freq, bw, tsamp, dm, 0.004)).cuda()
    multi = _run_lt(cfg, info, raw, nblocks, targets)
    assert len(multi) == ntarget
    if name == "L":
        assert all(len(m) > 1 for m in multi)
    single_cfg = pipeline.Config(**{**cfg.__dict__, "fused_fold": False})
    for k, t in enumerate(targets):
        _compare(multi[k], _run_lt(single_cfg, info, raw, nblocks, [t])[0])


def test_single_target_is_the_single_pulsar_path(gpu):
    from dspsr_amd import pipeline, synth
    freq, bw, tsamp, dm, nchan = 1382.0, -16.0, 1.0 / 32.0, 30.0, 16
    cfg = pipeline.Config(nchan=nchan, dispersion_measure=dm, nbin=64, folding_period=0.004, ndim=4, parts_per_block=3, max_parts=2)
    info = pipeline.InputInfo(centre_frequency=freq, bandwidth=bw, tsamp_us=tsamp)
    lt = pipeline.LoadToFold(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
    nblocks, step, overlap = 3, cfg.parts_per_block * lt.nsamp_step, lt.nsamp_overlap
    fused = lt.fused_fold
    lt.close()
    raw = torch.from_numpy(synth.voltages(nblocks * step + overlap, freq, bw, tsamp, dm, 0.004)).cuda()
    plain = _run_lt(cfg, info, raw, nblocks, None)
    one = _run_lt(pipeline.Config(**{**cfg.__dict__, "folding_period": 0.0, "nbin": 8}), info, raw, nblocks,
                  [pipeline.FoldTarget("a", folding_period=0.004, nbin=64)])
    assert len(one) == 1
    _compare(one[0], plain[0])
    lt = pipeline.LoadToFold(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream,
                             targets=[pipeline.FoldTarget("a", folding_period=0.004, nbin=64)])
    assert lt.fused_fold == fused and lt.pulsars == [] and lt.fold is not None
    lt.close()


def test_tool_writes_one_file_series_per_pulsar(gpu, tmp_path):
    """tools/dspsr_amd_fold.py with two -c: pulsar k writes <prefix>_<k>_<n>.ps with its own folding period in the header, and
    every file holds what the tool writes for that pulsar alone (<prefix>_<n>.ps).  The single-pulsar runs may take the fused
    fold, whose sums can be associated per run of parts (engine.fold_is_fused): profiles agree to float rounding, counts exactly."""
    import subprocess
    import sys
    from dspsr_amd import pipeline, synth
    freq, bw, tsamp, dm = 1382.0, -16.0, 1.0 / 32.0, 30.0
    raw = synth.voltages(400000, freq, bw, tsamp, dm, 0.004)
    path = tmp_path / "synthetic.dada"
    path.write_bytes(synth.dada_header(freq, bw, 1, 2, 1, tsamp) + raw.tobytes())
    periods = ["0.004", "0.00123"]

    def tool(prefix, *opts):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "dspsr_amd_fold.py"), "-F", "16:D", "-D", str(dm), "-b", "32", "-L", "0.004",
               *opts, "-O", str(tmp_path / prefix), str(path)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        return sorted(f for f in os.listdir(tmp_path) if f.startswith(prefix + "_") and f.endswith(".ps"))

    multi = tool("many", "-c", periods[0], "-c", periods[1])
    for k, period in enumerate(periods):
        mine = [f for f in multi if f.startswith("many_%d_" % k)]
        alone = tool("one%d" % k, "-c", period)
        assert len(mine) == len(alone) >= 2
        for n, (fm, fa) in enumerate(zip(mine, alone)):
            assert fm == "many_%d_%04d.ps" % (k, n) and fa == "one%d_%04d.ps" % (k, n)
            hm, hits_m, prof_m = pipeline.read_phase_series(str(tmp_path / fm))
            ha, hits_a, prof_a = pipeline.read_phase_series(str(tmp_path / fa))
            assert float(hm["FOLDING_PERIOD"]) == float(period) == float(ha["FOLDING_PERIOD"])
            assert {key: hm[key] for key in ("NBIN", "NDAT_TOTAL", "INTEGRATION_LENGTH", "DIVISION")} == \
                   {key: ha[key] for key in ("NBIN", "NDAT_TOTAL", "INTEGRATION_LENGTH", "DIVISION")}
            assert np.array_equal(hits_m, hits_a) and int(hits_m.sum()) == int(hm["NDAT_TOTAL"])
            assert np.abs(prof_m - prof_a).max() <= 1e-5 * np.abs(prof_a).max()
    assert len(multi) == sum(1 for f in multi if re.match(r"many_[01]_\d{4}\.ps$", f))
