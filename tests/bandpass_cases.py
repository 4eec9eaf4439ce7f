"""The cases of the passband kernels' device tests (tests/test_gpu_bandpass.py), built without a device so that the host suite can
check what the bit-for-bit comparison rests on (tests/test_bandpass_cases_host.py)."""
import functools

import numpy as np

import rfi_reference as rr

SENTINEL_UNITS = 5            # the passband holds 5 resolution^2 everywhere before a call: an exact value like the sums
RAW_SCALE = 2.0               # (int8 + 0.5) * 2 = odd integers

# (form, ndim, resolution, npol_in, npol_out, nchan_in, tone, big): form "float" / "generic" / "caspsr"; tone "dc" or "half" (the
# half-band tone of tests/plfb_cases.py: (-1)^t for Analytic rows, cos(pi t / 2) for Nyquist float rows; the 8-bit forms cannot hold a
# zero, their Nyquist half-band tone is a, a', -a, -a').  Every case runs the part counts 1, Tp - 1, Tp, Tp + 1 and 2 Tp + 1 (Tp = 8192
# / resolution parts per tile; three tiles = three segments, the last of one tile); `big` adds 256 Tp + 1: 257 tiles in 129 segments
# of two tiles, the last of one.
EXACT = [
    ("float", 1, 2, 2, 4, 1, "half", False),
    ("float", 2, 2, 2, 2, 3, "dc", False),
    ("float", 1, 16, 1, 1, 3, "dc", False),
    ("float", 2, 16, 2, 4, 1, "half", False),
    ("float", 1, 512, 2, 2, 1, "half", True),
    ("float", 2, 512, 2, 4, 3, "dc", False),
    ("float", 1, 1024, 2, 4, 1, "dc", True),
    ("float", 2, 1024, 1, 1, 1, "half", False),
    ("float", 1, 8192, 2, 4, 3, "half", False),
    ("float", 2, 8192, 2, 2, 1, "dc", False),
    ("float", 1, 8192, 1, 1, 1, "dc", False),
    ("generic", 1, 2, 2, 2, 3, "dc", False),
    ("generic", 1, 16, 1, 1, 1, "half", False),
    ("generic", 2, 16, 2, 4, 1, "half", False),
    ("generic", 2, 512, 1, 1, 3, "dc", False),
    ("generic", 1, 1024, 2, 4, 1, "half", False),
    ("generic", 2, 1024, 2, 2, 1, "dc", True),
    ("generic", 1, 8192, 2, 2, 3, "dc", False),
    ("generic", 2, 8192, 2, 4, 1, "half", False),
    ("caspsr", 1, 2, 2, 4, 1, "dc", False),
    ("caspsr", 1, 16, 2, 2, 1, "half", False),
    ("caspsr", 1, 512, 2, 4, 1, "half", False),
    ("caspsr", 1, 1024, 2, 2, 1, "dc", True),
    ("caspsr", 1, 8192, 2, 4, 1, "half", False),
]
IDS = ["%s-ndim%d-res%d-pol%dto%d-chan%d-%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], "-big" if c[7] else "") for c in EXACT]


def part_counts(index):
    res, big = EXACT[index][2], EXACT[index][7]
    tp = 8192 // res
    counts = [1, tp - 1, tp, tp + 1, 2 * tp + 1] + ([256 * tp + 1] if big else [])
    return sorted({c for c in counts if c >= 1})


def launch_arithmetic(npart, nchan_in, resolution):
    """(parts per tile, tiles per segment, segments): the cut of csrc/bandpass.hip restated from its description -- whole tiles
    per segment, about 1024 workgroups per launch, at most 256 segments, partial arrays within 256 MiB counted for four output
    polarisations (set_shape refuses nchan_in * resolution > 2^24, where one partial array alone would exceed that); a function of
    (npart, nchan_in, resolution) alone."""
    tp = 8192 // resolution
    ntile = -(-npart // tp)
    nseg = min(1024 // nchan_in, 256, (256 << 20) // (4 * nchan_in * resolution * 4), ntile)
    nseg = max(nseg, 1)
    tps = max(-(-ntile // nseg), 1)
    return tp, tps, -(-ntile // tps)


@functools.lru_cache(maxsize=None)
def exact_case(index, npart):
    """rows (float64 [nchan_in][npol_in][ndat * ndim], NaN in the trailing partial transform) or the byte block (uint8, -128 there),
    ndat, the float64 reference [npol_out][nchan_in][resolution]"""
    form, ndim, res, npol_in, npol_out, nchan_in, tone, _big = EXACT[index]
    rng = np.random.default_rng(1000 * index + npart % 997)
    nsamp_fft = res * (2 if ndim == 1 else 1)
    t = np.arange(nsamp_fft)
    if form == "float":
        amp = rng.integers(-3, 4, (nchan_in, npol_in, npart, 2))
        amp[..., 0] += (amp[..., 0] == 0) * 2
        if tone == "dc":
            tv = np.ones(nsamp_fft)
        else:
            tv = np.where(t % 2 == 0, 1.0, -1.0) if ndim == 2 else np.array([1.0, 0.0, -1.0, 0.0])[t % 4]
        body = np.empty((nchan_in, npol_in, npart, nsamp_fft, ndim))
        for d in range(ndim):
            body[..., d] = amp[..., d, None] * tv
        tail = nsamp_fft - 1
    else:
        amp = 2 * rng.integers(-3, 3, (nchan_in, npol_in, npart, 2)) + 1          # odd: what (int8 + 0.5) * 2 can hold
        body = np.empty((nchan_in, npol_in, npart, nsamp_fft, ndim))
        if ndim == 2:
            sign = np.ones(nsamp_fft) if tone == "dc" else np.where(t % 2 == 0, 1.0, -1.0)
            for d in range(2):
                body[..., d] = amp[..., d, None] * sign
        else:
            sign = np.ones(nsamp_fft) if tone == "dc" else np.where((t // 2) % 2 == 0, 1.0, -1.0)
            body[..., 0] = np.where(t % 2 == 0, amp[..., 0, None], amp[..., 1, None]) * sign
        tail = nsamp_fft - 2 if form == "caspsr" else nsamp_fft - 1
    ndat = npart * nsamp_fft + tail
    body = body.reshape(nchan_in, npol_in, npart * nsamp_fft * ndim)
    ref = rr.bandpass_loop(body, ndim, res, npol_out, np.float64, strict=False)
    if form == "float":
        rows = np.full((nchan_in, npol_in, ndat * ndim), np.nan)
        rows[:, :, :body.shape[2]] = body
        return rows, ndat, ref
    ndat_buf = ndat + (-ndat) % 4
    codes = np.full((nchan_in, npol_in, ndat_buf, ndim), -128, dtype=np.int64)
    codes[:, :, :npart * nsamp_fft, :] = np.rint((body.reshape(nchan_in, npol_in, npart * nsamp_fft, ndim) / RAW_SCALE) - 0.5)
    raw = rr.encode_raw(codes, form)
    return raw, ndat, ref


NOISE = [(1, 2, 4100), (2, 2, 8200), (1, 1024, 70), (2, 1024, 70), (1, 8192, 64), (2, 8192, 64)]      # (ndim, resolution, parts)


@functools.lru_cache(maxsize=None)
def noise_case(ndim, res, npart, seed=11):
    """Gaussian rows [2][2][ndat * ndim] -> four products; (rows float32, ndat, float64 reference, error figure of the float32
    strict-order restatement)"""
    rng = np.random.default_rng(seed + res + ndim)
    nsamp_fft = res * (2 if ndim == 1 else 1)
    ndat = npart * nsamp_fft + nsamp_fft // 2
    rows = rng.standard_normal((2, 2, ndat * ndim)).astype(np.float32)
    ref = rr.bandpass_loop(rows, ndim, res, 4, np.float64)
    f32 = rr.bandpass_loop(rows, ndim, res, 4, np.float32)
    assert f32.dtype == np.float32
    e_f32 = np.abs(f32.astype(np.float64) - ref).max() / np.abs(ref).max()
    return rows, ndat, ref, e_f32
