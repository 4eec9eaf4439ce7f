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
