"""The mask of tests/device_buffers.py (which floats of a sentinel buffer a correct writer touches) for every layout that
tests/test_gpu_output_forms.py builds: the right number of floats, all inside the view, and exactly the floats that the layout
include/dspsr_amd.h documents -- element (chan, plane, part, i) at first + chan * chan_stride + plane * pol_stride + part * part_step + i
-- receives.  Runs without a GPU."""
import numpy as np

import output_forms
from device_buffers import GUARD_FLOATS, OutputLayout, SENTINEL, describe_float, place_parts, written_mask


def test_every_layout_of_the_output_tests_masks_exactly_what_the_documented_layout_writes():
    n_layouts = 0
    for name, lay, npart, part_step, part_floats in output_forms.all_layouts():
        m = written_mask(lay, npart, part_step, part_floats)
        assert m.shape == (lay.size,) and m.sum() == lay.nchan * lay.nplanes * npart * part_floats, name
        w = lay.row + lay.row_pad
        # inside the view: between row (0, 0) and the end of the last row's data; guards of >= 256 bytes on both sides
        assert lay.first >= GUARD_FLOATS and lay.size - (lay.first + lay.nchan * lay.nplanes * w) >= GUARD_FLOATS, name
        if m.any():
            idx = np.flatnonzero(m)
            assert idx[0] == lay.first and idx[-1] < lay.first + lay.nchan * lay.nplanes * w - lay.row_pad, name
        # rows do not overlap in either order, and every row starts `offset` floats past a multiple of the row pitch
        span = (lay.nplanes - 1) * lay.pol_stride + w if not lay.plane_major else (lay.nchan - 1) * lay.chan_stride + w
        assert (lay.pol_stride if lay.plane_major else lay.chan_stride) >= span, name
        bits = np.full(lay.size, SENTINEL, np.int32)
        values = np.arange(1, 1 + lay.nchan * lay.nplanes * npart * part_floats, dtype=np.int32).reshape(lay.nchan, lay.nplanes, npart, part_floats)
        place_parts(lay, bits, values, part_step)
        assert np.array_equal(bits != SENTINEL, m), name
        assert np.array_equal(np.sort(bits[m]), values.ravel()), name                   # every value landed, once
        n_layouts += 1
    assert n_layouts >= 150


def test_layout_strides_and_descriptions():
    cm, pm = OutputLayout(3, 2, 20, offset=1, row_pad=3), OutputLayout(3, 2, 20, offset=1, row_pad=3, plane_major=True)
    assert (cm.chan_stride, cm.pol_stride) == (46, 23) and (pm.chan_stride, pm.pol_stride) == (23, 69)
    assert cm.first == pm.first == GUARD_FLOATS + 1
    # two parts of 6 floats, 8 apart, in rows of 20 + 3 floats
    for lay, chan, plane in ((cm, 1, 1), (pm, 1, 1)):
        r0 = lay.first + chan * lay.chan_stride + plane * lay.pol_stride
        assert "(chan 1, plane 1, float 0) inside part 0" in describe_float(lay, r0, 2, 8, 6)
        assert "float 6) inside the gap behind part 0" in describe_float(lay, r0 + 6, 2, 8, 6)
        assert "float 13) inside part 1" in describe_float(lay, r0 + 13, 2, 8, 6)
        assert "float 14) behind the last part" in describe_float(lay, r0 + 14, 2, 8, 6)
        assert "float 20) in the padding behind the row" in describe_float(lay, r0 + 20, 2, 8, 6)
        assert "guard in front of the rows, 1 floats" in describe_float(lay, lay.first - 1, 2, 8, 6)
        assert "guard behind the rows, 1 floats" in describe_float(lay, lay.first + 6 * 23, 2, 8, 6)
