"""The complex gain of every bin of every filterbank path against float64 (tests/transfer_cases.py: periodic input, an M-point DFT of the
output on the host; the method and the table are checked without a GPU by tests/test_transfer_cases_host.py).  One ordinary call of
perform_raw / perform per case into plain rows; the detected, fold and search forms are held bit for bit to this output elsewhere.

Per case: the output finite; the per-bin error rms and the worst bin within MARGIN times the same figure of the float32 oracle, both
relative to the rms bin amplitude; bin 0 of every channel and polarisation inside the same bound, asserted on its own so that a failure
names it.  The cases `fallback` names are held to the project's transform tolerance per bin and to an evenly spread error instead.
Every line printed ends in the three ratios to the float32 oracle; profiles/HISTORY.md holds the table."""
import numpy as np
import pytest

import transfer_cases as tc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MARGIN = 4                      # over the float32 oracle, as tests/test_gpu_spectral_truth.py
# A bin index or a channel whose error rms is more than SPREAD times that of all bins: structure, not rounding.  The mean of n >= 8
# squared errors of evenly spread noise (the windows of a case see the same rounding, so n counts a third of the samples at worst: 8 / 3
# independent complex errors, a Gamma(2.7) variable in units of its mean / 2.7) exceeds 9 times its expectation with probability
# < 1e-8 per group; one bin index holding a defect of the size of MARGIN times the oracle's worst bin exceeds it at once.
SPREAD = 3


def fallback(c):
    """Cases measured above MARGIN with no defect (profiles/HISTORY.md has the figures), named by what sets them apart; their worst bin is
    held to the transform tolerance 2e-6 sqrt(log2 2N) -- a bound of the project's, an eighth of _fb_case's, not one fitted to the
    device -- and their error must be spread evenly over bin indices and channels.  (reason, rms_too) or None; rms_too: the rms
    figure leaves MARGIN as well.
      * freq_res 1 and 2: the oracle's backward transform is a copy or one addition, so its float32 error is its forward transform's
        alone, 2.5e-8 ... 5e-8 rms where every other case has 0.7e-7 ... 2.4e-7; the device's 0.9e-7 ... 1.9e-7 is what it has at
        every length (its passes have the same stages whatever the lengths).  Ratios 2.8 ... 4.7, rms and worst bin alike.
      * an odd factor R >= 97 of nchan_subband: k_sub_combine_any adds the R sub-spectra of a bin one after the other into one float32
        accumulator, so its rounding grows with R where pocketfft's does not: the rms ratio rises evenly from 1.5 (R = 3) to 3.3
        (R = 127) and stays under MARGIN, which these cases still assert; the worst of ~10^4 bins then lands at 2.6 ... 4.6 times
        the oracle's worst, in a channel and a bin that differ from case to case."""
    if c["M"] <= 2:
        return "freq_res <= 2: the float32 oracle has no backward transform to round", True
    if c["family"] == "odd_C" and c["picks"]["nsub"] >= 97:
        return "k_sub_combine_any: a serial float32 sum of R >= 97 terms", False
    return None


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


def run_case(gpu, b):
    """the case's call on the device: complex128 [nchan][npol][npart * nkeep]"""
    dspsr_amd, ctx = gpu
    c, plan = b.case, b.plan
    eng = dspsr_amd.FilterbankEngine(ctx).setup(c["C"], c["M"], c["nfilt"][0], c["nfilt"][1], c["input_nchan"], c["npol"], c["real"],
                                                b.kernel, max_parts=c["max_parts"], force_four_pass=c["four"],
                                                split_in_inverse=c["sii"], response_matrix=b.matrix8)
    try:
        assert (eng.nsamp_fft, eng.nsamp_overlap, eng.nsamp_step, eng.nkeep) == \
            (plan.nsamp_fft, plan.nsamp_overlap, plan.nsamp_step, plan.nkeep)
        # the restatement the table was built from is what the library does
        assert eng.npass(c["form"] != "float") == c["picks"]["npass"], (eng.npass(c["form"] != "float"), c["picks"])
        assert eng.presplit() == c["picks"]["presplit"]
        assert eng.response_ndim() == (8 if c["matrix"] else 2 if c["kernel"] else 0)
        out = torch.zeros((plan.nchan, c["npol"], 2 * c["npart"] * plan.nkeep), dtype=torch.float32, device="cuda")
        if b.raw is not None:
            layout = dspsr_amd.RAW_CASPSR if c["form"] == "caspsr" else dspsr_amd.RAW_GENERIC
            eng.perform_raw(torch.from_numpy(b.raw).cuda(), layout, b.scale, out, c["npart"])
        else:
            eng.perform(torch.from_numpy(b.rows).cuda(), out, c["npart"], plan.nsamp_step * b.obs.ndim, 2 * plan.nkeep)
        eng.finish()
        return out.cpu().numpy().view(np.complex64)
    finally:
        eng.close()


@pytest.mark.parametrize("name", tc.NAMES)
def test_every_bin_against_float64(gpu, name):
    b, T, f32 = tc.truth(name)
    c = b.case
    got = run_case(gpu, b)
    assert np.isfinite(got.view(np.float32)).all()
    f = tc.figures(tc.gains(got, c), T)
    w, chan, pol, m = f["where"]
    by_m, at_m, by_s, at_s, n_m, n_s = tc.structure(f["err"])
    print("%s L=%d f32: rms %.3g worst %.3g bin0 %.3g  gpu: rms %.3g worst %.3g (window %d channel %d pol %d bin %d) bin0 %.3g  tol %.3g  "
          "spread m %.2f s %.2f  ratios rms %.2f worst %.2f bin0 %.2f" %
          (name, c["picks"]["L"], f32["rms"], f32["worst"], f32["bin0"], f["rms"], f["worst"], w, chan, pol, m, f["bin0"], tc.fb_tolerance(c),
           by_m, by_s, f["rms"] / f32["rms"], f["worst"] / f32["worst"], f["bin0"] / f32["worst"]))
    err0 = f["err"][..., 0]
    w0, chan0, pol0 = (int(i) for i in np.unravel_index(int(np.argmax(err0)), err0.shape))
    fb = fallback(c)
    if fb is not None:
        tol = tc.fb_tolerance(c)
        print("    fallback (%s): worst / tol %.3f; error rms by bin index at most %.2f (m = %d, %d samples), by channel at most %.2f "
              "(channel %d, %d samples) of the rms of all" % (fb[0], f["worst"] / tol, by_m, at_m, n_m, by_s, at_s, n_s))
        assert fb[1] or f["rms"] <= MARGIN * f32["rms"], "per-bin error rms %.3g > %d x %.3g" % (f["rms"], MARGIN, f32["rms"])
        assert f["worst"] <= tol, "bin %d of channel %d, polarisation %d (window %d) is off by %.3g > %.3g" % (m, chan, pol, w, f["worst"], tol)
        assert f["bin0"] <= tol, "bin 0 of channel %d, polarisation %d (window %d) is off by %.3g > %.3g" % (chan0, pol0, w0, f["bin0"], tol)
        # (a group of fewer than 8 samples says nothing about its rms)
        assert n_m < 8 or by_m <= SPREAD, "bin index %d carries %.2f times the error rms of all" % (at_m, by_m)
        assert n_s < 8 or by_s <= SPREAD, "channel %d carries %.2f times the error rms of all" % (at_s, by_s)
        return
    assert f["rms"] <= MARGIN * f32["rms"], "per-bin error rms %.3g > %d x %.3g" % (f["rms"], MARGIN, f32["rms"])
    assert f["worst"] <= MARGIN * f32["worst"], \
        "bin %d of channel %d, polarisation %d (window %d) is off by %.3g of the rms amplitude > %d x %.3g" % (m, chan, pol, w, f["worst"],
                                                                                                          MARGIN, f32["worst"])
    assert f["bin0"] <= MARGIN * f32["worst"], \
        "bin 0 of channel %d, polarisation %d (window %d) is off by %.3g of the rms amplitude > %d x %.3g" % (chan0, pol0, w0, f["bin0"],
                                                                                                           MARGIN, f32["worst"])
