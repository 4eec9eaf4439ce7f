"""GUPPI / PUPPI raw files, restated independently of dspsr_amd.guppi and of the kernel: the address of every byte written out,
one element at a time.

A file is a sequence of blocks: a header of 80-character cards `KEYWORD = value` closed by an END card, then BLOCSIZE bytes.  The
data section holds nchan runs of chan_stride = BLOCSIZE / nchan bytes; run c holds the consecutive samples of channel c, 2 * npol
int8 each ((re, im) of polarisation 0, then of polarisation 1).  The last OVERLAP samples of a run repeat the first samples of the
next block and are never delivered: a block delivers block_nsamp = chan_stride / (2 npol) - OVERLAP samples.
    byte of kept sample s of (chan c, pol p) of block b = b * block_stride + c * chan_stride + (s * npol + p) * 2 + d
Value = float(int8): no half step, no scale."""
import numpy as np

# (block_nsamp, OVERLAP): runs of 1024 bytes at npol 2; of 1056; of 1028 (npol 2) / 514 (npol 1): not 16-byte aligned, and not 4-byte
# aligned at npol 1
GEOMETRIES = [(256, 0), (259, 5), (255, 2)]


def chan_stride_of(block_nsamp, overlap, npol):
    return (block_nsamp + overlap) * 2 * npol


def stream_from_blocks(blocks, nchan, npol, block_nsamp, overlap, chan_stride=None, block_stride=None):
    """int8 bytes of whole data sections -> complex64 [nchan][npol][nblk * block_nsamp], the stream in time order as float(int8).
    chan_stride / block_stride: bytes between runs / data sections where they are not the packed ones"""
    blocks = np.asarray(blocks).reshape(-1).view(np.int8)
    cs = chan_stride_of(block_nsamp, overlap, npol) if chan_stride is None else chan_stride
    bs = nchan * cs if block_stride is None else block_stride
    nblk = -(-blocks.size // bs)
    assert (nblk - 1) * bs + (nchan - 1) * cs + block_nsamp * 2 * npol <= blocks.size
    out = np.zeros((nchan, npol, nblk * block_nsamp), np.complex64)
    s = np.arange(block_nsamp)
    for b in range(nblk):
        for c in range(nchan):
            for p in range(npol):
                at = b * bs + c * cs + (s * npol + p) * 2           # the address of every kept sample, element by element
                out[c, p, b * block_nsamp + s] = blocks[at].astype(np.float32) + 1j * blocks[at + 1].astype(np.float32)
    return out


def rows_of(stream, first, ndat):
    """float32 rows [nchan][npol][2 * ndat] of samples first ... first + ndat - 1 of stream_from_blocks' result"""
    s = np.ascontiguousarray(stream[:, :, first:first + ndat])
    assert s.shape[2] == ndat
    return s.view(np.float32).reshape(s.shape[0], s.shape[1], 2 * ndat).copy()


def random_blocks(nbytes, seed=0):
    return np.random.default_rng(seed).integers(-128, 128, nbytes, dtype=np.int8)


def random_samples(nchan, npol, ndat, seed=0):
    """int8 [nchan][npol][ndat][2]"""
    return np.random.default_rng(seed).integers(-128, 128, (nchan, npol, ndat, 2), dtype=np.int8)


def complex_of(x):
    """int8 [nchan][npol][ndat][2] -> complex64 [nchan][npol][ndat] as float(int8)"""
    return (x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)).astype(np.complex64)


def data_section(x, k, block_nsamp, overlap, seed=1234):
    """the data section of stream block k of x (int8 [nchan][npol][ndat][2]): samples k * block_nsamp ... + block_nsamp + overlap - 1 of
    every channel, the overlap being the next block's first samples; what lies past the end of x is random filler"""
    nchan, npol, ndat, _ = x.shape
    n = block_nsamp + overlap
    run = np.random.default_rng(seed + k).integers(-128, 128, (nchan, npol, n, 2), dtype=np.int8)
    have = max(0, min(n, ndat - k * block_nsamp))
    run[:, :, :have] = x[:, :, k * block_nsamp:k * block_nsamp + have]
    return np.ascontiguousarray(run.transpose(0, 2, 1, 3)).reshape(-1)          # [chan][sample][pol][2]


CARDS = {"BACKEND": "GUPPI", "TELESCOP": "GBT", "FRONTEND": "Rcvr_800", "SRC_NAME": "B0329+54", "RA_STR": "03:32:59.3680",
         "DEC_STR": "+54:34:43.5700", "FD_POLN": "LIN", "OBSFREQ": 820.0, "OBSBW": -16.0, "OBSNCHAN": 4, "NPOL": 4, "NBITS": 8, "TBIN": 2.5e-07,
         "PKTFMT": "1SFA", "PKTSIZE": 8192, "OVERLAP": 0, "BLOCSIZE": 0, "STT_IMJD": 55555, "STT_SMJD": 43200, "STT_OFFS": 0.25, "PKTIDX": 0}


def header(cards):
    """the cards as FITS-style text, 80 characters each, strings in single quotes, closed by END"""
    out = b""
    for key, v in cards.items():
        text = ("'%-8s'" % v) if isinstance(v, str) else repr(v) if isinstance(v, float) else "%d" % v
        card = ("%-8s= %s" % (key, text if isinstance(v, str) else "%20s" % text)).encode("ascii")
        assert len(key) <= 8 and len(card) <= 80
        out += card + b" " * (80 - len(card))
    return out + b"END" + b" " * 77


def write_raw(path, x, block_nsamp, overlap, *, seq=None, packets_per_block=4, cards=None, drop=(), lead=None, tail=b""):
    """A raw file of the samples x (int8 [nchan][npol][ndat][2]): one block per entry (k, pktidx) of `seq` -- stream block k of x with
    that PKTIDX (default: every whole block of x in sequence, PKTIDX k * packets_per_block); k None: a data section of zero bytes.
    cards: keywords to override or add; drop: keywords to leave out; lead: (cards, data bytes) of a block in front of all;
    tail: bytes behind the last block.  Returns the cards of the first block of `seq`."""
    nchan, npol, ndat, _ = x.shape
    cs = chan_stride_of(block_nsamp, overlap, npol)
    kept = block_nsamp * 2 * npol * nchan
    assert kept % packets_per_block == 0
    if seq is None:
        seq = [(k, k * packets_per_block) for k in range(ndat // block_nsamp)]
    base = dict(CARDS, OBSNCHAN=nchan, NPOL=4 if npol == 2 else 1, OVERLAP=overlap, BLOCSIZE=nchan * cs, PKTSIZE=kept // packets_per_block)
    base.update(cards or {})
    for key in drop:
        del base[key]
    with open(path, "wb") as f:
        if lead is not None:
            f.write(header(lead[0]))
            f.write(np.asarray(lead[1]).view(np.int8).tobytes())
        for k, pktidx in seq:
            f.write(header(dict(base, PKTIDX=pktidx)))
            f.write((np.zeros(nchan * cs, np.int8) if k is None else data_section(x, k, block_nsamp, overlap)).tobytes())
        f.write(tail)
    return dict(base, PKTIDX=seq[0][1])


def stream_of_file(f, nchan, npol):
    """complex64 [nchan][npol][nstream * block_nsamp]: every stream block of the open dspsr_amd.guppi.GuppiFile `f`, as its blocks()
    would deliver them to a driver that asks for everything -- read through sections(), unpacked by the restatement"""
    n = len(f.stream)
    return stream_from_blocks(f.sections(0, n), nchan, npol, f.block_nsamp, f.overlap) if n else np.zeros((nchan, npol, 0), np.complex64)


class Driver:
    """the geometry a driver shows to blocks(): parts_per_block parts of nsamp_step samples and nsamp_overlap behind them, of blocks
    in the form `form` (dspsr_amd.inputs: the file's own)"""

    def __init__(self, parts_per_block, nsamp_step, nsamp_overlap, form):
        from types import SimpleNamespace
        self.form = form
        self.cfg = SimpleNamespace(parts_per_block=parts_per_block)
        self.nsamp_step, self.nsamp_overlap = nsamp_step, nsamp_overlap
