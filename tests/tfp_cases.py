"""The launch arithmetic of dspsr_amd_tfp_filterbank (dspsr_amd/csrc/tfp.hip, the function at the end of the file) restated on the
host, and the cases of tests/test_gpu_tfp.py built from it.  Kept free of torch so that tests/test_tfp_dispatch_model.py can check
on a machine without a GPU that the cases reach what they are there for.

The three kernel families are persistent: grid = min(nitem, ncu), a workgroup walks item = blockIdx.x, += gridDim.x, prefetches
the first tile of its NEXT item while it post-processes the last tile of the current one, and restarts its time-scrunch sums per
item.  A case tests that only when nitem > ncu -- so every count below is a function of the device's ncu."""
from collections import namedtuple

K_TFP_COAL, K_TFP_HALF, K_TFP4K, K_TFPM = "k_tfp coalesced", "k_tfp half-word", "k_tfp4k", "k_tfpm"
FAMILIES = (K_TFP_COAL, K_TFP_HALF, K_TFP4K, K_TFPM)
TILE_BYTES = 1 << 15              # one workgroup tile: 2^14 points = T parts x 2 polarisations x 2 nchan samples, one byte each
ALL_NCHAN = tuple(1 << k for k in range(4, 14))

# family None: nothing is launched -- `refused` holds the text of the EINVAL, or None when the call has nothing to do (nout = 0)
Dispatch = namedtuple("Dispatch", "family T groups_per_out nout nitem grid refused")


def dispatch(nchan, tscrunch, npart, caspsr, align, ncu, npol=2):
    """What dspsr_amd_tfp_filterbank does with a block whose first byte lies `align` bytes behind a 16-byte boundary, in the
    order of its checks."""
    def refuse(text):
        return Dispatch(None, 0, 0, 0, 0, 0, text)
    if nchan < 16 or nchan & (nchan - 1) or nchan > 8192:
        return refuse("nchan=%d must be a power of two in [16, 8192]" % nchan)
    if npol != 2:
        return refuse("only real dual-polarisation 8-bit input is built (npol=%d)" % npol)
    sf = tscrunch or 1
    T = 8192 // nchan                                       # parts per tile: 1 << (14 - log2 nchan - 1)
    if sf % T and T % sf:
        return refuse("tscrunch=%d must divide or be a multiple of %d parts per workgroup" % (sf, T))
    if align & 1:                                           # both byte orders are read as half words
        return refuse("raw pointer must be 2-byte aligned")
    nout = npart // sf
    if nout == 0:
        return Dispatch(None, T, 0, 0, 0, 0, None)
    coal = align % 16 == 0
    family = K_TFP_COAL if coal else K_TFP_HALF
    if nchan == 4096 and coal and sf % 2 == 0:
        family = K_TFP4K
    if coal and sf % T == 0 and nchan in (512, 1024, 2048, 8192):
        family = K_TFPM
    groups_per_out = sf // T if sf > T else 1
    nitem = nout if sf > T else (nout * sf + T - 1) // T
    return Dispatch(family, T, groups_per_out, nout, nitem, min(nitem, ncu), None)


def items_wanted(ncu):
    """2.5 items per workgroup and one more: the first ncu // 2 + 1 workgroups take three items, the others two"""
    return 2 * ncu + ncu // 2 + 1


def npart_for(nchan, tscrunch, nitem, ragged=True):
    """parts that give `nitem` work items.  tscrunch >= T: nitem whole output samples and, where the factor leaves room, a tail
    that completes none.  tscrunch < T: the last tile holds ONE output sample (the kernel stops inside the tile), and a tail."""
    sf, T = tscrunch or 1, 8192 // nchan
    nout = nitem if sf >= T else ((nitem - 1) * T) // sf + 1
    return nout * sf + ((sf - 1 if sf < 8 else sf // 2 + 1) if ragged and sf > 1 else 0)


Case = namedtuple("Case", "nchan tscrunch caspsr pscrunch npart align")


def case_id(c):
    """without npart, the one field that depends on the device: the same ids on every machine"""
    return "%d-t%d-%s-%s-a%d" % (c.nchan, c.tscrunch, "caspsr" if c.caspsr else "generic", "psc" if c.pscrunch else "ppqq", c.align)


def half_word_align(caspsr):
    """a block that only the half-word k_tfp takes: 2-byte aligned (generic order), 8-byte aligned (CASPSR groups of 4 + 4)"""
    return 8 if caspsr else 2


def anchor_cases(ncu):
    """the half-word generic kernel at tscrunch 1, every channel count, both byte orders, 2.5 items per workgroup with a last
    tile that is half empty; pscrunch alternates with the channel count (and, per channel count, with the byte order)"""
    out = []
    for k, nchan in enumerate(ALL_NCHAN):
        T = 8192 // nchan
        npart = (items_wanted(ncu) - 1) * T + (T + 1) // 2
        for caspsr in (False, True):
            out.append(Case(nchan, 1, caspsr, bool((k + caspsr) & 1), npart, half_word_align(caspsr)))
    return out


_FORMS = ((False, True), (True, False), (False, False), (True, True))        # (caspsr, pscrunch), dealt in turn


def exact_cases(ncu):
    """every path that must give the bits of the anchor kernel's per-part powers summed in time order: (nchan, tscrunch, align)
    by family, the byte order and pscrunch dealt in turn WITHIN a family (each family sees the four combinations), npart from
    the model: 2.5 items per workgroup, a ragged tail wherever the factor leaves room for one"""
    N = items_wanted(ncu)
    shapes = {
        # T = 2: groups_per_out 1, 3, 8 (the benchmark's factor), 2
        K_TFP4K: [(4096, 2), (4096, 6), (4096, 16), (4096, 4), (4096, 6), (4096, 16), (4096, 2), (4096, 10)],
        # tscrunch = T and a multiple of T (8192: T = 1, every factor -- an odd one included); in this order every channel count
        # meets the four combinations of byte order and pscrunch
        K_TFPM: [(512, 16), (512, 32), (1024, 8), (1024, 24), (2048, 4), (2048, 12), (8192, 1), (8192, 3),
                 (1024, 16), (1024, 8), (512, 48), (512, 16), (8192, 2), (8192, 5), (2048, 8), (2048, 4)],
        # tscrunch < T, == T, > T where the host leaves an aligned block to k_tfp: below 512 channels all three, 512 ... 2048
        # below T only, 4096 with tscrunch 1 only, 8192 never (T = 1 divides every factor: k_tfpm)
        K_TFP_COAL: [(16, 1), (16, 64), (16, 512), (16, 1024), (32, 2), (32, 256), (32, 768), (64, 4), (64, 128), (64, 256),
                     (128, 1), (128, 16), (128, 64), (128, 192), (256, 8), (256, 32), (256, 64), (512, 1), (512, 4), (512, 8),
                     (1024, 2), (1024, 4), (1024, 1), (2048, 1), (2048, 2), (4096, 1), (4096, 1)],
        # the anchor kernel itself at other factors
        K_TFP_HALF: [(16, 128), (16, 1024), (64, 2), (64, 128), (256, 96), (512, 8), (1024, 8), (2048, 2), (2048, 8),
                     (4096, 2), (4096, 16), (8192, 3), (8192, 4), (128, 32), (32, 256), (4096, 6)],
    }
    out = []
    for family, lst in shapes.items():
        for i, (nchan, sf) in enumerate(lst):
            caspsr, psc = _FORMS[i % 4]
            align = half_word_align(caspsr) if family == K_TFP_HALF else 0
            out.append(Case(nchan, sf, caspsr, psc, npart_for(nchan, sf, N), align))
    return out


def bench_case(ncu):
    """the benchmarked geometry (digifil -F 4096 -t 16, PPQQ into Rescale) scaled to the device: eight output samples per workgroup"""
    return Case(4096, 16, False, False, 16 * 8 * ncu, 0)


# CASPSR blocks 2, 4 and 8 bytes behind a 16-byte boundary against the aligned block, at a factor that sends the aligned block
# to each of the three families
def caspsr_offset_cases(ncu):
    N = items_wanted(ncu)
    return [Case(nchan, sf, True, psc, npart_for(nchan, sf, N), align)
            for (nchan, sf, psc) in ((4096, 2, True), (1024, 8, False), (128, 16, True)) for align in (2, 4, 8)]


def all_cases(ncu):
    return anchor_cases(ncu) + exact_cases(ncu) + [bench_case(ncu)] + caspsr_offset_cases(ncu)


def chain_case(ncu):
    """LoadToFil at scale: (nchan, tscrunch, parts_per_block) with more than two output samples per workgroup in each block"""
    return 1024, 8, 8 * items_wanted(ncu)


def anchor_block(nchan, npart, seed):
    """the noise of the anchor cases: Gaussian of 24 levels rms, clipped to int8, npart parts of 2 * nchan samples x 2 polarisations"""
    import numpy as np
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.standard_normal(npart * 4 * nchan, dtype=np.float32) * np.float32(24.0)), -128, 127).astype(np.int8)


def mirror_bins(nchan):
    """bins 0 and nchan / 2 are their own mirrors in the real-transform split and take code of their own in all three kernel
    families; with them their neighbours and the far end of the band"""
    return [0, 1, nchan // 2 - 1, nchan // 2, nchan // 2 + 1, nchan - 1]
