"""Device buffers for the GPU tests: float rows placed away from the allocator's alignment, with a sentinel around them."""
import numpy as np

GUARD_ALIGN = 256


def device_rows(x, offset, row_pad):
    """float32 [nchan][npol][n] rows as a strided view: `offset` floats past a 256-byte boundary, rows `row_pad` floats longer than
    their data (channel and polarisation strides n + row_pad), the rest of the buffer NaN"""
    import torch
    nchan, npol, n = x.shape
    w = n + row_pad
    buf = torch.full((GUARD_ALIGN + offset + nchan * npol * w + GUARD_ALIGN,), float("nan"), dtype=torch.float32, device="cuda")
    lead = ((-buf.data_ptr()) % GUARD_ALIGN) // 4
    rows = buf[lead + offset:lead + offset + nchan * npol * w].view(nchan, npol, w)[:, :, :n]
    assert rows.data_ptr() % GUARD_ALIGN == (4 * offset) % GUARD_ALIGN and rows.stride() == (npol * w, w, 1)
    rows.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return rows


# ---- output side: rows cut from a buffer that holds one bit pattern no kernel produces ----------------------------------------
SENTINEL = 0x7fc0dead           # a quiet NaN with a payload: compared as BITS (int32 views), never as floats
GUARD_FLOATS = GUARD_ALIGN // 4


class OutputLayout:
    """Where a [nchan][nplanes][row] view lies in a buffer of `size` floats: element (c, p, i) at first + c * chan_stride +
    p * pol_stride + i.  Channel-major: pol_stride = row + row_pad, chan_stride = nplanes * pol_stride; plane-major (the second
    order dspsr_amd_filterbank_perform_detect accepts): chan_stride = row + row_pad, pol_stride = nchan * chan_stride.  `first` is
    `offset` floats past a 256-byte boundary with at least GUARD_FLOATS floats in front, and as many behind the last row."""

    def __init__(self, nchan, nplanes, row, offset=0, row_pad=0, plane_major=False, lead=GUARD_FLOATS):
        w = row + row_pad
        self.nchan, self.nplanes, self.row, self.offset, self.row_pad, self.plane_major = nchan, nplanes, row, offset, row_pad, plane_major
        self.chan_stride, self.pol_stride = (w, nchan * w) if plane_major else (nplanes * w, w)
        self.first = lead + offset
        self.size = self.first + nchan * nplanes * w + GUARD_FLOATS

    def where(self, index):
        """(chan, plane, float within the row, "inside a row" | "behind a row") of buffer index `index`, or (None, None, distance
        from the rows, "guard"); describe_float tells a part from a gap"""
        w = self.row + self.row_pad
        k = index - self.first
        if k < 0 or k >= self.nchan * self.nplanes * w:
            return None, None, k if k < 0 else k - self.nchan * self.nplanes * w, "guard"
        r, i = divmod(k, w)
        chan, plane = (r % self.nchan, r // self.nchan) if self.plane_major else (r // self.nplanes, r % self.nplanes)
        return chan, plane, i, "inside a row" if i < self.row else "behind a row"


def written_mask(lay, npart, part_step, part_floats):
    """bool[lay.size]: the floats a correct writer touches when it puts `npart` parts of `part_floats` floats, `part_step` floats
    apart, into every row of the layout (include/dspsr_amd.h: row(c, p) + part * part_step + [0, part_floats))"""
    m = np.zeros(lay.size, bool)
    assert npart == 0 or (part_step >= part_floats and (npart - 1) * part_step + part_floats <= lay.row)
    for c in range(lay.nchan):
        for p in range(lay.nplanes):
            r0 = lay.first + c * lay.chan_stride + p * lay.pol_stride
            for k in range(npart):
                m[r0 + k * part_step:r0 + k * part_step + part_floats] = True
    return m


def place_parts(lay, bits, values, part_step):
    """the layout of include/dspsr_amd.h written out: values int32 [nchan][nplanes][npart][part_floats] put into bits[lay.size]
    at row(c, p) + part * part_step, one element at a time (no slices: an emulation of the address arithmetic, not of the mask)"""
    nchan, nplanes, npart, n = values.shape
    i = np.arange(n)
    for c in range(nchan):
        for p in range(nplanes):
            for k in range(npart):
                bits[lay.first + c * lay.chan_stride + p * lay.pol_stride + k * part_step + i] = values[c, p, k]
    return bits


def describe_float(lay, index, npart, part_step, part_floats):
    """a buffer index as text: (chan, plane, float within row) and where it lies relative to what a correct writer touches"""
    chan, plane, i, where = lay.where(index)
    if where == "inside a row":
        k, j = divmod(i, part_step) if part_step else (0, i)
        if npart and k < npart and j < part_floats:
            where = "inside part %d" % k
        elif npart and k < npart - 1:
            where = "inside the gap behind part %d" % k
        else:
            where = "behind the last part of the row" if npart else "inside a row of an empty call"
    elif where == "behind a row":
        where = "in the padding behind the row (in front of the next row)"
    elif where == "guard":
        where = "in the guard %s the rows, %d floats from them" % (("in front of", -i) if i < 0 else ("behind", i + 1))
    return "buffer float %d = (chan %s, plane %s, float %s) %s" % (index, chan, plane, i, where)


def sentinel_rows(lay):
    """(buf, rows): a device buffer of lay.size floats (plus slack to align it) that holds SENTINEL everywhere, as int32, and the
    float32 view [nchan][nplanes][row] of the layout; buf[i] is the layout's buffer index i"""
    import torch
    raw = torch.full((lay.size + GUARD_FLOATS,), SENTINEL, dtype=torch.int32, device="cuda")
    skew = ((-raw.data_ptr()) % GUARD_ALIGN) // 4
    buf = raw[skew:skew + lay.size]
    w = lay.row + lay.row_pad
    body = buf[lay.first:lay.first + lay.nchan * lay.nplanes * w].view(torch.float32)
    rows = body.view(lay.nplanes, lay.nchan, w).permute(1, 0, 2) if lay.plane_major else body.view(lay.nchan, lay.nplanes, w)
    rows = rows[:, :, :lay.row]
    assert rows.data_ptr() % GUARD_ALIGN == (4 * lay.offset) % GUARD_ALIGN and rows.stride() == (lay.chan_stride, lay.pol_stride, 1)
    return buf, rows
