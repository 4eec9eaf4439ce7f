"""The cases of tests/test_gpu_search_forms.py as plain data, with their references: the stand-alone search-mode operations digifil
runs behind the filterbank (csrc/scrunch.hip, csrc/sample_delay.hip, csrc/rescale.hip) on rows placed as dsp::TimeSeries places them.
Kept free of torch so that tests/test_search_forms_host.py can check on a machine without a GPU everything that needs no device.

Exact data.  exact_block() returns float32 values that are integer multiples of 2^-g (g = granule_bits) below 2^m (m = max_bits).
Every x, and every float32 product x*x (a rounded product of two such numbers is still a multiple of 2^-2g), is then a multiple of a
fixed power of two, and a sum of n of them needs at most ceil(log2 n) + 2m + 2g bits: while that is <= 52 every partial sum is exact
in double, whatever the order of addition.  Rescale's total and totalsq are then the same numbers on the GPU (tree sums) and in the
reference (sample by sample); mean, variance (rounded product, rounded difference), 1/sqrt and the float conversions are IEEE
operations with one correct result -- offset, scale, every output float and every packed byte must equal the oracle's, no tolerance."""
import math

import numpy as np

import oracle.dspsr_oracle as _o
from device_buffers import OutputLayout

EXACT_BITS = 52


def bit_budget(nsum, granule_bits, max_bits):
    """bits the sum of `nsum` squares of exact_block values can need"""
    return max(0, math.ceil(math.log2(max(1, nsum)))) + 2 * max_bits + 2 * granule_bits


def exact_block(rng, shape, gain, granule_bits=8, max_bits=7, nsum=1):
    """float32 g*z^2 + g (z normal; gain scalar or broadcastable) rounded to multiples of 2^-granule_bits, magnitudes below
    2^max_bits.  nsum: the largest number of samples a case adds into one sum -- outside the exact regime this raises."""
    assert granule_bits + max_bits <= 24, "a value would not fit a float32"
    assert bit_budget(nsum, granule_bits, max_bits) <= EXACT_BITS, \
        "sums of %d samples (granule 2^-%d, below 2^%d) need %d bits: not exact in double" % (
            nsum, granule_bits, max_bits, bit_budget(nsum, granule_bits, max_bits))
    g = np.asarray(gain, np.float32)
    x = (rng.standard_normal(shape).astype(np.float32) ** 2 * g + g).astype(np.float64)
    q = 2.0 ** granule_bits
    lim = 2.0 ** max_bits - 1.0 / q
    return np.clip(np.rint(x * q) / q, -lim, lim).astype(np.float32)


# ---- placements: (offset, row_pad, plane_major) of the input rows, the same of the output rows.  Offsets 0-3 and row_pad 0 / 1 / 3 on
# either side, the two sides independent, one plane-major layout (pol_stride > chan_stride) on each side
PLACEMENTS = [((0, 0, False), (2, 1, False)), ((1, 3, False), (3, 0, False)), ((2, 1, True), (0, 3, False)), ((3, 0, False), (1, 1, True))]


def layout(nchan, npol, row, place):
    offset, row_pad, plane_major = place
    return OutputLayout(nchan, npol, row, offset, row_pad, plane_major)


# ---- dsp::TScrunch, FPT ------------------------------------------------------------------------------------------------------------
def tscrunch_ref(x, sf, ndim):
    """oracle.tscrunch_fpt with the ndim axis moved next to the polarisations: rows [nchan][npol][ndat * ndim] ->
    [nchan][npol * ndim][ndat] -> scrunch -> back.  (Every dimension is scrunched on its own, TScrunch.C:148-178.)"""
    x = np.asarray(x, np.float32)
    nchan, npol, nfloat = x.shape
    ndat = nfloat // ndim
    planes = x.reshape(nchan, npol, ndat, ndim).transpose(0, 1, 3, 2).reshape(nchan, npol * ndim, ndat)
    out = _o.tscrunch_fpt(planes, sf)
    return np.ascontiguousarray(out.reshape(nchan, npol, ndim, -1).transpose(0, 1, 3, 2)).reshape(nchan, npol, -1)


def stream_reference(x, blocks, sf, ndim):
    """per call of a stream (x: rows [nchan][npol][sum(blocks) * ndim] cut into calls of blocks[k] samples): dict(c0, nout, carry_count,
    out = float32 [nchan][npol][nout * ndim], carry = float32 [nchan][npol][ndim], the sequential float sum of the samples behind the
    last complete output -- None when the call leaves no such samples: the carry buffer is then not touched)"""
    x = np.asarray(x, np.float32)
    nchan, npol, _ = x.shape
    full = tscrunch_ref(x, sf, ndim).reshape(nchan, npol, -1, ndim)
    samples = x.reshape(nchan, npol, -1, ndim)
    calls, pos = [], 0
    for n in blocks:
        o0, o1, rem = pos // sf, (pos + n) // sf, (pos + n) % sf
        carry = None
        if rem and n:
            s0 = pos + n - rem
            carry = samples[:, :, s0].copy()
            for i in range(s0 + 1, pos + n):
                carry = carry + samples[:, :, i]                         # float32, in stream order
        calls.append(dict(c0=pos % sf, nout=o1 - o0, carry_count=rem, carry=carry,
                          out=np.ascontiguousarray(full[:, :, o0:o1]).reshape(nchan, npol, -1)))
        pos += n
    return calls


# (name, nchan, npol, ndim, sfactor, samples per call, placement) -- k_tscrunch_fpt, csrc/scrunch.hip:12-54
TSCRUNCH_CASES = [
    # ndim 1: calls that end inside an output (1000), begin and end inside one (37), close one exactly (3: rem 0), complete none
    # without (8) and with (the last 3) a carry in front, and 312 outputs -- more than a workgroup -- behind a carry
    ("ndim1", 5, 1, 1, 16, (1000, 37, 3, 8, 5001, 3), 0),
    # ndim 2 (Coherence / Stokes with ndim 2: HIP::TScrunchEngine passes in->get_ndim()): the carry is [row][ndim], scrunch.hip:36,47,50
    ("ndim2", 3, 2, 2, 7, (100, 5, 1, 1, 9, 1000, 2, 7), 1),
    # ndim 4: 91 outputs x 4 dimensions = more (o, d) pairs than a workgroup holds, scrunch.hip:27-29
    ("ndim4", 4, 1, 4, 3, (274, 1, 1, 823, 1000, 2, 2), 2),
    ("ndim2-planes-out", 3, 2, 2, 5, (64, 3, 2, 131), 3),
    # beyond the grid cap (scrunch.hip:94-95, 1024 blocks x 256 threads): 150 000 outputs x 2 dimensions per row, the walk-on loop :27
    ("beyond-grid-cap", 1, 2, 2, 2, (300001, 2), 1),
]

# (name, nchan, npol, nfloat, sfactor, placement) -- k_fscrunch_fpt, csrc/scrunch.hip:56-70; nfloat no multiple of 256
FSCRUNCH_CASES = [("sf%d-place%d" % (sf, p), 6, 2, 1001, sf, p) for sf, p in ((1, 0), (2, 1), (3, 2), (6, 3), (2, 2), (3, 0))]
# plane-major input (placement 2): f * ics walks the SHORT stride, scrunch.hip:62,66
# beyond the grid cap (scrunch.hip:119-120): more than 1024 x 256 floats per row
FSCRUNCH_CASES += [("beyond-grid-cap", 2, 1, 1024 * 256 + 257, 2, 1)]

# ---- dsp::SampleDelay -- k_sample_delay, csrc/sample_delay.hip:22-48 (chunks of 2048 floats; out of place the rows are cut into
# segments, :144-156; in place one workgroup walks the whole row).  (name, nchan, npol, ndim, nout, absolute, in place, placement)
SAMPLE_DELAY_CASES = [
    ("2047", 3, 2, 1, 2047, False, False, 0), ("2048", 3, 2, 1, 2048, False, False, 1), ("2049", 3, 2, 1, 2049, True, False, 2),
    ("2047-inplace", 3, 2, 1, 2047, False, True, 1), ("2049-inplace", 3, 2, 1, 2049, True, True, 2),
    ("ndim2-2048", 4, 2, 2, 1024, False, False, 3), ("ndim2-2050-inplace", 4, 2, 2, 1025, False, True, 3),
    ("ndim4-2052", 5, 1, 4, 513, True, False, 0), ("ndim4-2044-inplace", 5, 1, 4, 511, False, True, 0),
    # nseg 4, the last segment of 100 floats (sample_delay.hip:154-156)
    ("ragged-segments", 3, 2, 1, 3 * 2048 + 100, False, False, 1),
    ("ragged-segments-ndim2", 3, 2, 2, 3 * 1024 + 51, True, False, 2),
    # 1024 rows: two segments of three and of two-and-a-bit chunks each -- the chunk loop :34 out of place; in place: six chunks per row
    ("chunk-loop", 512, 2, 1, 5 * 2048 + 7, False, False, 1), ("chunk-loop-inplace", 8, 2, 2, 5 * 1024 + 3, False, True, 2),
]
SAMPLE_DELAY_MAX = 40


def sample_delays(rng, nchan, npol, absolute):
    """delays [nchan][npol] that include 0 and SAMPLE_DELAY_MAX (relative: per channel, as Dedispersion::SampleDelay gives them)"""
    d = rng.integers(0, SAMPLE_DELAY_MAX + 1, (nchan, npol if absolute else 1))
    d.flat[0], d.flat[-1] = 0, SAMPLE_DELAY_MAX
    return np.ascontiguousarray(np.broadcast_to(d, (nchan, npol))).astype(np.int64)


# ---- dsp::Rescale + dsp::SigProcDigitizer (+ dsp::PScrunch) on exact_block data ------------------------------------------------------
NBITS = (1, 2, 4, 8, 16)
# name: (nchan, npol, samples per block, interval, constant, flip, swap, (granule_bits, max_bits), which kernel / line it is there for)
# nchan: a multiple of 8 (one-bit samples, rescale.hip:487,529,578) that is no multiple of 64 (the tile of k_digitize_fpt, :215-223)
RESCALE_CASES = {
    # intervals that end inside a block and span blocks (777 = 7 x 100 + 77); 80 columns: one ragged tile of 256 (rescale.hip:30-31)
    "ends-inside": (40, 2, (777, 777, 500), 100, False, True, False, (8, 7), "rescale.hip:343-381 interval segments"),
    # an interval longer than a block, Coherence (npol 4: xpol_offset for ipol > 1, rescale.hip:121,233); 288 columns: two tiles
    "exceeds-block": (72, 4, (300, 300, 700), 1000, False, False, True, (8, 7), "rescale.hip:345-346,372-373"),
    # interval 0 = the first block's length (:339), constant: the later estimates are computed and dropped (:375)
    "interval0-constant": (264, 1, (513, 200, 513), 0, True, True, True, (8, 7), "rescale.hip:339,375 set_scale"),
    "interval0": (24, 2, (300, 300), 0, False, False, False, (8, 7), "rescale.hip:339"),
}
# beyond the grid caps; each (nchan, npol, blocks, interval, ...) as above
RESCALE_BIG = {
    # k_rescale_apply_fpt, rescale.hip:567-568: 256 blocks x 256 threads per row
    "apply-fpt-cap": (2, 1, (70001,), 0, False, False, False, (8, 7), "rescale.hip:201 walk-on loop"),
    # k_rescale_pscrunch_digitize, rescale.hip:502: gridDim.y 8192 rows
    # (one launch per interval segment, :343-381: interval 0 = the block's 9000 rows in ONE segment, two trips of the loop)
    "fused-rows-cap": (16, 2, (9000, 8200), 0, False, True, False, (8, 7), "rescale.hip:459 walk-on loop"),
    # a small block, then one interval of more than 64 x 4096 rows on the same object: part_sum / part_sq regrow (rescale.hip:352-361)
    # and rows_per_block doubles (:351); TFP
    "tfp-slices-double": (2, 2, (100, 64 * 4096 + 69), 64 * 4096 + 69, False, False, False, (8, 7), "rescale.hip:349-361"),
    # the same for one FPT row of more than 4096 x 4096 samples (67 MB)
    "fpt-slices-double": (1, 1, (1000, 4096 * 4096 + 4099), 4096 * 4096 + 4099, False, False, False, (8, 5), "rescale.hip:349-361"),
}
# k_sigproc_digitize / k_sigproc_float / k_pscrunch_tfp, rescale.hip:278,522,537: 8192 blocks x 256 threads, fewer than the units
DIGITIZE_BIG = dict(nchan=64, npol=2, ndat=33000)
assert DIGITIZE_BIG["nchan"] * DIGITIZE_BIG["ndat"] > 8192 * 256


def rescale_case(name):
    return RESCALE_CASES[name] if name in RESCALE_CASES else RESCALE_BIG[name]


def rescale_intervals(blocks, interval):
    """[(start, end)] in stream samples of every run of samples Rescale sums into one total before it computes (or, `constant`,
    drops) an estimate, and the run left open at the end (Rescale.C:217-326): the first block's first segment, then `nsample` each"""
    nsample = interval or blocks[0]
    runs, pos, begin, isample, first = [], 0, 0, 0, True
    for ndat in blocks:
        start = 0
        while start < ndat:
            end = min(ndat, start + nsample - isample)
            isample += end - start
            if isample == nsample or first:
                runs.append((begin, pos + end))
                begin, isample, first = pos + end, 0, False
            start = end
        pos += ndat
    if begin < pos:
        runs.append((begin, pos))
    return runs


def rescale_pieces(blocks, interval):
    """[(start, end)] in stream samples of every segment Rescale hands to one apply launch: the part of a run that lies in one
    block (rescale.hip:343-381)"""
    bounds = [0] + list(np.cumsum(blocks))
    return [(max(s, b0), min(e, b1)) for s, e in rescale_intervals(blocks, interval) for b0, b1 in zip(bounds, bounds[1:])
            if max(s, b0) < min(e, b1)]


def rescale_blocks(name):
    """the blocks of a case in TFP order, float32 [ndat][nchan][npol] each, exact for the longest run the case sums; column (0, 0) of
    the first block is constant: zero variance, scale 1 (Rescale.C:411-412)"""
    nchan, npol, blocks, interval, _, _, _, (gran, maxb), _ = rescale_case(name)
    nsum = max(e - s for s, e in rescale_intervals(blocks, interval))
    rng = np.random.default_rng(abs(hash_name(name)))
    out = []
    for b, ndat in enumerate(blocks):
        gain = rng.uniform(0.5, 2.0 ** maxb / 12.0, (1, nchan, npol)).astype(np.float32)
        x = exact_block(rng, (ndat, nchan, npol), gain, gran, maxb, nsum)
        if b == 0:
            x[:, 0, 0] = 3.0
        out.append(x)
    return out


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def packed_bytes(ndat, nchan, npol, nbit):
    return ndat * nchan * npol * (32 if nbit == -32 else nbit) // 8


# ---- which kernel is reached where: (placed rows, beyond its grid cap or walk-on loop) -----------------------------------------------
KERNELS = {
    "k_tscrunch_fpt": ("TSCRUNCH_CASES ndim1/2/4", "TSCRUNCH_CASES beyond-grid-cap"),
    "k_fscrunch_fpt": ("FSCRUNCH_CASES", "FSCRUNCH_CASES beyond-grid-cap"),
    "k_sample_delay": ("SAMPLE_DELAY_CASES", "SAMPLE_DELAY_CASES chunk-loop (no grid cap can be reached: nseg <= 2048)"),
    "k_rescale_sums": ("RESCALE_CASES, TFP", "RESCALE_BIG tfp-slices-double"),
    "k_rescale_sums_fpt": ("RESCALE_CASES, FPT", "RESCALE_BIG fpt-slices-double"),
    "k_rescale_accumulate": ("RESCALE_CASES", "RESCALE_BIG *-slices-double (more than 4096 slices asked for)"),
    "k_rescale_update": ("RESCALE_CASES", "RESCALE_CASES exceeds-block, interval0-constant (more than 256 columns)"),
    "k_rescale_apply": ("RESCALE_CASES, TFP", "RESCALE_BIG tfp-slices-double (more than 4096 x 256 floats)"),
    "k_rescale_apply_fpt": ("RESCALE_CASES, FPT", "RESCALE_BIG apply-fpt-cap, fpt-slices-double"),
    "k_sigproc_digitize": ("RESCALE_CASES, TFP", "DIGITIZE_BIG"),
    "k_sigproc_float": ("RESCALE_CASES, TFP", "DIGITIZE_BIG"),
    "k_pscrunch_tfp": ("RESCALE_CASES ends-inside, interval0", "DIGITIZE_BIG"),
    "k_digitize_fpt": ("RESCALE_CASES, FPT", "not here: tests/test_gpu_search.py test_fpt_kernels_beyond_the_grid_limits (65535 time tiles, contiguous rows)"),
    "k_rescale_pscrunch_digitize": ("RESCALE_CASES ends-inside, interval0", "RESCALE_BIG fused-rows-cap"),
}
