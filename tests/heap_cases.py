"""The MeerKAT beamformer's heap order (INSTRUMENT MKBF / MKBFRo), restated independently of dspsr_amd.dada and of the kernels: plain
loops over heap, polarisation, channel and sample, one byte at a time.

A block is whole heaps of 256 samples.  Heap h holds, for pol in order and then chan in order, the 256 consecutive complex samples
of that (chan, pol) as (int8 re, int8 im) pairs:
    byte of stored sample s of heap h = (((h * npol + pol) * nchan + chan) * 256 + s) * 2 + d
Stream sample t of a row is stored at s = t & 255 of heap t >> 8 (MKBF) or at s = (t & 255) ^ 1 (MKBFRo, odd and even samples
exchanged).  Value = (float(int8) + 0.5f) * scale."""
import numpy as np

HEAP = 256
MACHINES = {"MKBF": False, "MKBFRo": True}      # machine -> odd and even samples exchanged


def heap_bytes(nheap, nchan, npol):
    return nheap * npol * nchan * HEAP * 2


def stream_from_heaps(block, nchan, npol, swap):
    """int8 bytes of whole heaps -> int8 [nchan][npol][nheap * 256][2], the stream samples in time order"""
    block = np.asarray(block).reshape(-1).view(np.int8)
    nheap = block.size // heap_bytes(1, nchan, npol)
    assert nheap * heap_bytes(1, nchan, npol) == block.size
    out = np.zeros((nchan, npol, nheap * HEAP, 2), np.int8)
    for h in range(nheap):
        for pol in range(npol):
            for chan in range(nchan):
                for s in range(HEAP):
                    t = h * HEAP + ((s ^ 1) if swap else s)           # the stream sample stored at s
                    for d in range(2):
                        out[chan, pol, t, d] = block[(((h * npol + pol) * nchan + chan) * HEAP + s) * 2 + d]
    return out


def heaps_from_stream(x, swap):
    """int8 [nchan][npol][ndat][2] (ndat a multiple of 256) -> the bytes of the block of heaps"""
    nchan, npol, ndat, _ = x.shape
    assert ndat % HEAP == 0
    block = np.zeros(heap_bytes(ndat // HEAP, nchan, npol), np.int8)
    for t in range(ndat):
        h, s = t >> 8, (t & 255) ^ (1 if swap else 0)
        for pol in range(npol):
            for chan in range(nchan):
                for d in range(2):
                    block[(((h * npol + pol) * nchan + chan) * HEAP + s) * 2 + d] = x[chan, pol, t, d]
    return block


def rows_of(stream, first_sample, ndat, scale):
    """float32 rows [nchan][npol][2 * ndat] of samples first_sample ... first_sample + ndat - 1 of stream_from_heaps' result"""
    s = stream[:, :, first_sample:first_sample + ndat]
    assert s.shape[2] == ndat
    v = (s.astype(np.float32) + np.float32(0.5)) * np.float32(scale)
    return np.ascontiguousarray(v.reshape(s.shape[0], s.shape[1], 2 * ndat)).astype(np.float32)


def unpack(block, nchan, npol, swap, first_sample, ndat, scale):
    """float32 rows [nchan][npol][2 * ndat]: stream samples first_sample ... first_sample + ndat - 1 of the block"""
    return rows_of(stream_from_heaps(block, nchan, npol, swap), first_sample, ndat, scale)


def random_block(nheap, nchan, npol, seed=0):
    return np.random.default_rng(seed).integers(-128, 128, heap_bytes(nheap, nchan, npol), dtype=np.int8)


def write_dada(path, block, *, machine, nchan, npol, freq=1382.0, bw=-16.0, tsamp_us=0.25, ndim=2, nbit=8, extra=None):
    """a DADA file: 4096-byte header (INSTRUMENT `machine`) + the bytes of `block`"""
    from dspsr_amd import synth
    hdr = synth.dada_header(freq, bw, nchan, npol, ndim, tsamp_us, instrument=machine, extra=extra)
    if nbit != 8:
        hdr = hdr.replace(b"NBIT 8", b"NBIT %d" % nbit)
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(np.asarray(block).view(np.int8).tobytes())
    return str(path)
