"""SIGPROC filterbank input: a loop restatement of dsp::SigProcUnpacker::unpack, OrderFPT branch (sigproc/SigProcUnpacker.C:98-153),
the case tables of the kernel test, and the small files the host and pipeline tests fold.  numpy only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NBITS = (1, 2, 4, 8, 16, 32)
NPOLS = (1, 2, 4)
NDATS = (1, 3, 63, 64, 65, 257, 1000)            # below, at and one past the tile of 64 spectra; several tiles; a ragged end


def spectrum_bytes(nbit, nchan, npol):
    assert (npol * nchan * nbit) % 8 == 0
    return npol * nchan * nbit // 8


def unpack_fpt(raw, nbit, nchan, npol, ndat):
    """SigProcUnpacker.C:98-153 row by row: raw = uint8[ndat * S]; returns float32 [nchan][npol][ndat].  The walk over time is a
    strided slice, everything else is the reference's own arithmetic: from = from_base + ((ipol * nchan + ichan) >> div_shift),
    shift = (ichan & mod_mask) * nbit, keep_mask, the offset of the rows ipol > 1, a step of nchan_bytes * npol bytes -- or of
    nchan * npol elements of 16 or 32 bits -- from a spectrum to the next."""
    raw = np.ascontiguousarray(raw, np.uint8)
    div_shift, mod_mask, keep_mask = {1: (3, 0x07, 0x01), 2: (2, 0x03, 0x03), 4: (1, 0x01, 0x0f)}.get(nbit, (0, 0, 0xff))
    nchan_bytes = nchan >> div_shift
    assert raw.size == ndat * spectrum_bytes(nbit, nchan, npol)
    out = np.zeros((nchan, npol, ndat), np.float32)
    from32 = np.frombuffer(raw.tobytes(), "<f4") if nbit == 32 else None
    from16 = np.frombuffer(raw.tobytes(), "<u2") if nbit == 16 else None
    for ipol in range(npol):
        offset = np.float32(0.0)
        if nbit == 16 and ipol > 1:
            offset = np.float32(32768.0)
        if nbit == 8 and ipol > 1:
            offset = np.float32(127.5)
        for ichan in range(nchan):
            if nbit == 32:
                out[ichan, ipol] = from32[nchan * ipol + ichan::nchan * npol][:ndat]
            elif nbit == 16:
                out[ichan, ipol] = from16[ipol * nchan + ichan::nchan * npol][:ndat].astype(np.float32) - offset
            elif nbit == 8:
                out[ichan, ipol] = raw[ipol * nchan + ichan::nchan * npol][:ndat].astype(np.float32) - offset
            else:
                start = (ipol * nchan + ichan) >> div_shift
                shift = (ichan & mod_mask) * nbit
                out[ichan, ipol] = ((raw[start::nchan_bytes * npol][:ndat] >> shift) & keep_mask).astype(np.float32)
    return out


def random_spectra(nbit, nchan, npol, ndat, seed=0):
    """uint8[ndat * S]: random bytes; nbit 32: random finite floats of every magnitude, with a NaN, an infinity, a negative zero and
    a denormal among the first values (compared as bit patterns)"""
    rng = np.random.default_rng(1000 * nbit + 10 * nchan + npol + 7 * ndat + seed)
    n = ndat * spectrum_bytes(nbit, nchan, npol)
    if nbit != 32:
        return rng.integers(0, 256, n, dtype=np.uint8)
    bits = rng.integers(0, 1 << 32, n // 4, dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7f800000) == 0x7f800000] &= 0x3fffffff                  # the random ones are finite
    special = np.array([0x7fc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x7fa00000], np.uint32)
    k = min(special.size, bits.size)
    bits[rng.permutation(bits.size)[:k]] = special[:k]
    return bits.view(np.uint8).copy()


def smallest_nchan(nbit):
    """one byte per polarisation (sub-byte samples), else one value"""
    return max(8 // nbit, 1)


def raw_offsets(nbit):
    """the byte offsets 0 ... 15 at which the first spectrum may start"""
    return list(range(0, 16, max(nbit // 8, 1)))


def kernel_cases(nbit):
    """[(nchan, npol, ndat, raw byte offset, row offset in floats, row padding)] of the kernel test for one sample size.
    Every npol with every nchan of {smallest, 24, 40, 64, 200} (nbit 1 and nchan 8, 24: an odd spectrum; nbit 2 and nchan 24: an
    even one that is no multiple of 4) and every ndat of the list, the raw offsets and the row placements (16-byte aligned or not,
    padded or not) taken in turn; then the two shapes with whole tiles -- 200 x 1 (a tile and an edge along the spectrum) and 64 x 4 (two
    tiles) -- over 257 spectra at every raw offset, each on aligned rows and on rows of mixed alignment, so that every load width meets whole tiles, edge spectra and rows of both
    alignments; one case of 1024 channels."""
    offs, places = raw_offsets(nbit), [(0, 0), (1, 0), (0, 3), (2, 1), (3, 3), (0, 1)]
    cases, k = [], 0
    for npol in NPOLS:
        for nchan in (smallest_nchan(nbit), 24, 40, 64, 200):
            for ndat in NDATS:
                cases.append((nchan, npol, ndat, offs[(3 * k) % len(offs)]) + places[k % len(places)])
                k += 1
    for nchan, npol in ((200, 1), (64, 4)):
        for off in offs:
            cases.append((nchan, npol, 257, off, 0, 3))       # every row 16-byte aligned: float4 stores
            cases.append((nchan, npol, 257, off, 1, 0))       # one row in four is
    cases.append((1024, 2, 65, 0, 0, 0))
    return cases


def load_width(nbit, raw_address, S):
    """the load width a call takes (include/dspsr_amd.h): the widest of 16, 8, 4, 2, 1 bytes that divides the address and the spectrum,
    holds a value and is at most an eighth of the tile's 16 * nbit bytes"""
    a, most = raw_address | S, min(2 * nbit, 16)
    for w in (16, 8, 4, 2, 1):
        if w <= most and 8 * w >= nbit and a % w == 0:
            return w
    raise AssertionError("no load width for nbit %d at %d, S %d" % (nbit, raw_address, S))


LOAD_WIDTHS = {1: (1, 2), 2: (1, 2, 4), 4: (1, 2, 4, 8), 8: (1, 2, 4, 8, 16), 16: (2, 4, 8, 16), 32: (4, 8, 16)}


# ---- files ---------------------------------------------------------------------------------------------------------------------
HEADER = dict(source_name="J0000+0000", fch1=1500.0, foff=-0.5, tstart_mjd=56000.25, tsamp=64e-6)


def write_fil(path, data, *, nbits, nchans, nifs, **header):
    """A SIGPROC filterbank file: pipeline.write_sigproc_header and the bytes of `data` (any dtype) behind it.  Returns the header's
    length in bytes."""
    from dspsr_amd import pipeline
    h = dict(HEADER, nbits=nbits, nchans=nchans, nifs=nifs)
    h.update(header)
    with open(path, "wb") as f:
        pipeline.write_sigproc_header(f, **h)
        n = f.tell()
        f.write(np.ascontiguousarray(data).tobytes())
    return n


def pack(values, nbit):
    """values: integers (or, nbit 32, floats) [ndat][npol][nchan] -> the file's bytes; sub-byte values lowest bits first"""
    v = np.asarray(values)
    if nbit == 32:
        return v.astype("<f4").view(np.uint8).reshape(-1)
    if nbit == 16:
        return v.astype("<u2").view(np.uint8).reshape(-1)
    if nbit == 8:
        return v.astype(np.uint8).reshape(-1)
    spb = 8 // nbit
    g = v.astype(np.uint8).reshape(-1, spb)
    return (g << (np.arange(spb, dtype=np.uint8) * nbit)).sum(axis=1).astype(np.uint8)
