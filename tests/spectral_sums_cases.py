"""Seeded noise through the two transform-detect-add kernels (csrc/plfb.hip, csrc/bandpass.hip), for a comparison of bits between
commits: tools/spectral_sums_record.py runs every case and records a digest of the sums, tests/test_gpu_spectral_sums_parent.py runs
them again and compares.  The cases are built without a device (run_case alone needs one); tests/test_spectral_sums_cases_host.py
checks what the cases claim to reach.

Every case has 2 Tp + 1 parts (Bandpass) or windows (PLFB), Tp = 8192 / C of them per workgroup tile: three tiles, cut into three
segments of one tile, the last tile holding one part.  The tone cases of bandpass_cases.py and plfb_cases.py give sums that are exact
in any order; these do not: a sum taken in another order, or a product rounded elsewhere, changes the digest."""
import functools
import hashlib

import numpy as np

from bandpass_cases import RAW_SCALE

SIZES = (2, 16, 512, 2048, 4096, 8192)                 # 4096 and 8192: either side of k_bandpass's held / evaluated twiddles
ENDS = (16, 8192)

# (form, ndim, resolution, npol_in, npol_out); one input channel
BANDPASS = ([("float", d, c, 2, 4) for d in (1, 2) for c in SIZES] +
            [("float", d, c, pi, po) for d in (1, 2) for c in ENDS for pi, po in ((1, 1), (2, 2))] +
            [("generic", d, c, 2, 4) for d in (1, 2) for c in ENDS] +
            [("caspsr", 1, c, 2, 4) for c in (16, 1024, 8192)])
# (ndim, nchan, npol_in, npol_out); two input channels, five phase bins
PLFB = ([(d, c, 2, 4) for d in (1, 2) for c in SIZES] +
        [(d, c, pi, po) for d in (1, 2) for c in ENDS for pi, po in ((2, 1), (1, 1), (2, 2))])
PLFB_NCHAN_IN, PLFB_NBIN = 2, 5

BANDPASS_IDS = ["bandpass-%s-ndim%d-res%d-pol%dto%d" % c for c in BANDPASS]
PLFB_IDS = ["plfb-ndim%d-nchan%d-pol%dto%d" % c for c in PLFB]
IDS = BANDPASS_IDS + PLFB_IDS


def _seed(name):
    return [ord(ch) for ch in name]


@functools.lru_cache(maxsize=None)
def bandpass_case(index):
    """(rows float32 [1][npol_in][ndat * ndim], or the byte block uint8; ndat): 2 Tp + 1 parts and half a transform more"""
    form, ndim, res, npol_in, _npol_out = BANDPASS[index]
    rng = np.random.default_rng(_seed(BANDPASS_IDS[index]))
    nsamp_fft = res * (2 if ndim == 1 else 1)
    npart = 2 * (8192 // res) + 1
    ndat = npart * nsamp_fft + nsamp_fft // 2
    if form == "float":
        return rng.standard_normal((1, npol_in, ndat * ndim)).astype(np.float32), ndat
    # generic: [ndat][1][npol][ndim] bytes; CASPSR: whole groups of 4 + 4 bytes
    nbytes = ndat * npol_in * ndim if form == "generic" else -(-ndat // 4) * 8
    return rng.integers(0, 256, nbytes, dtype=np.uint8), ndat


def plfb_bins(nwin):
    """The bin of each of the 2 Tp + 1 windows: of the five bins at least one has windows either side of a segment boundary (its
    sums go through slots and k_plfb_combine) and at least one lies inside a segment (added to the profile directly)."""
    if nwin == 3:
        return np.array([0, 1, 0], dtype=np.uint32)
    if nwin == 5:
        return np.array([0, 2, 1, 0, 2], dtype=np.uint32)
    return ((3 * np.arange(nwin)) % PLFB_NBIN).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def plfb_case(index):
    """(rows float32 [2][npol_in][ndat * ndim], starts uint64, bins uint32, ndat): 2 Tp + 1 windows one sample apart"""
    ndim, nchan, npol_in, _npol_out = PLFB[index]
    rng = np.random.default_rng(_seed(PLFB_IDS[index]))
    nwin = 2 * (8192 // nchan) + 1
    starts = np.arange(nwin, dtype=np.uint64)
    ndat = nwin - 1 + nchan * (2 if ndim == 1 else 1)
    rows = rng.standard_normal((PLFB_NCHAN_IN, npol_in, ndat * ndim)).astype(np.float32)
    return rows, starts, plfb_bins(nwin), ndat


def plfb_cut(nwin, nchan_in, nchan, npol_out):
    """(windows per tile, windows per segment, segments): the cut of csrc/plfb.hip restated from its description -- whole tiles per
    segment, about 1024 workgroups per launch, at most 256 segments, two slots per segment within 256 MiB."""
    tp = 8192 // nchan
    ntile = -(-nwin // tp)
    nseg = max(min(1024 // nchan_in, 256, (256 << 20) // (2 * npol_out * nchan_in * nchan * 4), ntile), 1)
    wps = -(-ntile // nseg) * tp
    return tp, wps, -(-nwin // wps)


def plfb_bin_segments(bins, wps):
    """bin -> (first, last) segment of its windows in the bin-sorted list"""
    order = np.sort(np.asarray(bins), kind="stable")
    return {int(b): (int(np.flatnonzero(order == b)[0]) // wps, int(np.flatnonzero(order == b)[-1]) // wps) for b in np.unique(order)}


def run_case(dspsr_amd, ctx, name):
    """the sums of one case on the device, onto a zeroed array, public API only; float32 on the host"""
    import torch
    if name in BANDPASS_IDS:
        index = BANDPASS_IDS.index(name)
        form, ndim, res, npol_in, npol_out = BANDPASS[index]
        data, ndat = bandpass_case(index)
        dev = torch.from_numpy(data).cuda()
        eng = dspsr_amd.BandpassEngine(ctx)
        eng.set_shape(1, npol_in, ndim, res, npol_out)
        if form == "float":
            eng.accumulate(dev, ndat)
        else:
            eng.accumulate_raw(dev, ndat, dspsr_amd.RAW_CASPSR if form == "caspsr" else dspsr_amd.RAW_GENERIC, RAW_SCALE)
    else:
        index = PLFB_IDS.index(name)
        ndim, nchan, npol_in, npol_out = PLFB[index]
        rows, starts, bins, ndat = plfb_case(index)
        dev = torch.from_numpy(rows).cuda()
        eng = dspsr_amd.PhaseLockedFilterbankEngine(ctx)
        eng.set_shape(PLFB_NCHAN_IN, npol_in, ndim, nchan, npol_out, PLFB_NBIN)
        eng.accumulate(dev, ndat, starts, bins)
    got = eng.synch()
    eng.close()
    return got


def record_of(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "shape": list(a.shape), "first": [float(v).hex() for v in a.reshape(-1)[:8]]}
