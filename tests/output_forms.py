"""The cases of tests/test_gpu_output_forms.py as plain data: which object, which call, where the output rows lie.  Kept free of
torch so that tests/test_output_mask.py can check every layout's mask on a machine without a GPU.

An output row of dsp::TimeSeries starts at buffer + reserve and is padded (TimeSeries.C:146-179): as a rule 8-byte but not 16-byte
aligned, strides that are no multiples of 4 floats.  offset: floats between a 256-byte boundary and row (0, 0); row_pad: floats
between the end of a row and the next; step_extra: out_step - 2 * nkeep."""
from device_buffers import OutputLayout

# name: (C, M, nfilt, npart, _fb_block keywords, calls that reach the family, npass() that proves it ran: (raw_input, value))
# npart 3 with max_parts 2: a call spans a full launch group and a ragged one
FAMILIES = {
    # filterbank.hip fb_run_tiles, one inverse pass: inv_store of fb_inv_epilogue.h (float2 rows; float4 / float2 / planes)
    "inv_chan": (16, 256, (20, 21), 3, dict(max_parts=2), ("raw", "rows"), (1, 3)),
    # fb_run_tiles, four-pass inverse (k_inv_a + k_inv_b), forced: k_inv_b's store of fb_four_pass.hip (float2 rows; detected)
    "four_pass_forced": (16, 256, (20, 21), 3, dict(max_parts=2, four_pass=True), ("raw", "rows"), (1, 4)),
    # the same kernels by length (freq_res > 8192)
    "four_pass_long": (2, 16384, (900, 1100), 3, dict(max_parts=2), ("raw",), (1, 4)),
    # fb_run_two_pass (complex dual-pol 8-bit block, nchan_subband * freq_res^2 = 2^27): k_rows_inv of fb_two_pass.hip, the same inv_store
    "two_pass": (512, 512, (27, 27), 3, dict(real=False, max_parts=2), ("raw",), (1, 2)),
    # nchan_subband = 3 * 2^k: k_sub_split + k_sub_combine in front of the inverse pass of fb_inv_chan.h
    "odd_channels": (96, 256, (20, 21), 3, dict(max_parts=2), ("raw",), (1, 3)),
    # freq_res = 5 * 2^k: the last step is k_time_combine (fb_inv_chan.hip), which writes with the row writers of fb_common.h itself
    "odd_freq_res": (16, 5 * 128, (33, 20), 3, dict(max_parts=2), ("raw", "rows"), (1, 3)),
    # fb_run_subbands: two input channels, FbOut::chan0 moves the rows of the second
    "subbands": (16, 256, (20, 21), 3, dict(input_nchan=2, max_parts=2), ("raw",), (1, 3)),
    # fb_run_plain (freq_res = 1): fb_plain.hip:330-351; 64 parts of two polarisations per tile, 70 parts: a ragged second tile
    "plain": (64, 1, (0, 0), 70, dict(), ("raw", "rows"), (1, 1)),
    # fb_run_conv1 (n_fft <= 8192, float rows): fb_conv1.hip:134-140 (float2 rows), :150-153 (detected)
    "conv1": (1, 4096, (300, 301), 3, dict(real=False, input_nchan=3, max_parts=2, use_raw=False), ("rows",), (0, 1)),
    # fb_run_conv3, 2^14 points: fb_conv3.hip:78-98, 359-394 (buffer stores into the kept window), parts in two launch groups
    "conv3_14": (1, 16384, (1000, 900), 3, dict(real=False, input_nchan=3, max_parts=2, use_raw=False), ("rows",), (0, 3)),
    # fb_run_conv3, 2^17 points, max_parts 512: two channels per launch group, three channels -- a ragged last channel group
    "conv3_17": (1, 131072, (5000, 4000), 3, dict(real=False, input_nchan=3, max_parts=512, use_raw=False), ("rows",), (0, 3)),
    # fb_run_batched: four channels of a convolution as one launch group through the four-pass kernels (force_four_pass = 1)
    "batched": (1, 1024, (100, 90), 3, dict(real=False, input_nchan=4, max_parts=2, four_pass=True, use_raw=False), ("rows",), (0, 4)),
}
CONVOLUTIONS = ("conv1", "conv3_14", "conv3_17", "batched")


def geometry(family):
    """(output channels, nkeep, npart) of a family"""
    C, M, nfilt, npart, kw, _, _ = FAMILIES[family]
    return C * kw.get("input_nchan", 1), M - sum(nfilt), npart


# ---- complex rows: (offset, row_pad, step_extra); every offset 0-3, every row_pad 0 / 1 / 3, every out_step; (2, 0, .) is DSPSR's
# usual row (8-byte aligned), offsets 1 and 3 rows that are only float aligned
COMPLEX_FORMS = [(2, 0, 0), (0, 1, 2), (1, 3, 6), (3, 0, 2), (0, 0, 6), (2, 1, 0)]
# the convolutions' adaptor (host/dspsr_amd_engines.h ConvolutionEngine::perform) passes out_step = in_step; "fft": parts a whole
# transform apart (2 * freq_res floats), the largest gap a caller would leave
COMPLEX_CASES = [(f, call, off, pad, extra) for f in FAMILIES for call in FAMILIES[f][5] for off, pad, extra in COMPLEX_FORMS]
COMPLEX_CASES += [(f, "rows", 2, 0, extra) for f in CONVOLUTIONS for extra in ("in_step", "fft")]


def complex_layout(family, offset, row_pad, extra, npol=2, nparts_room=None):
    """(layout, npart, out_step, floats per part) of a complex-row case; nparts_room: parts the rows have room for (default npart)"""
    nchan, nkeep, npart = geometry(family)
    M, nfilt = FAMILIES[family][1], FAMILIES[family][2]
    step = 2 * nkeep + (0 if extra == "in_step" else 2 * sum(nfilt) if extra == "fft" else extra)
    room = npart if nparts_room is None else nparts_room
    return OutputLayout(nchan, npol, (room - 1) * step + 2 * nkeep, offset, row_pad), npart, step, 2 * nkeep


# ---- detected rows: every (family, ndim) at (offset 2, row_pad 0), (1, 3) and (0, 1), channel-major, the state alternating so that
# every (family, ndim) sees Coherence and Stokes; every family once plane-major (ndim 1 and 2 in turn, offset 3: the offset the
# channel-major forms leave out)
DETECT_FORMS = [(2, 0), (1, 3), (0, 1)]
DETECT_CASES = [(f, ndim, ("Coherence", "Stokes")[(i + j + k) % 2], off, pad, False)
                for i, f in enumerate(FAMILIES) for j, ndim in enumerate((1, 2, 4)) for k, (off, pad) in enumerate(DETECT_FORMS)]
DETECT_CASES += [(f, (2, 1)[i % 2], ("Stokes", "Coherence")[(i // 2) % 2], 3, (1, 0, 3)[i % 3], True) for i, f in enumerate(FAMILIES)]


def detect_layout(family, ndim, offset, row_pad, plane_major, nparts_room=None):
    """(layout, 1, row floats, row floats): a detected row is one run of npart * nkeep * ndim floats"""
    nchan, nkeep, npart = geometry(family)
    n = npart * nkeep * ndim
    room = n if nparts_room is None else nparts_room * nkeep * ndim
    return OutputLayout(nchan, 4 // ndim, room, offset, row_pad, plane_major), 1, n, n


# ---- search rows: (family, state, tscrunch); two calls of 2 and 3 parts, so that the second starts with a carry wherever
# 2 * nkeep is no multiple of the factor; rows with offset 1 and row_pad 1 that have room for one more output than a call writes
SEARCH_FAMILIES = ("inv_chan", "two_pass", "subbands", "four_pass_forced")       # the last: not fused (the internal detected block)
SEARCH_PARTS = (2, 3)
SEARCH_CASES = [(f, state, sf) for f in SEARCH_FAMILIES for state in ("Intensity", "PPQQ") for sf in (1, 3, 16)]


def search_layouts(family, state, sf):
    """[(layout, 1, nout, nout)] of the two calls of a search case"""
    nchan, nkeep, _ = geometry(family)
    out, cc = [], 0
    for npart in SEARCH_PARTS:
        nout = (cc + npart * nkeep) // sf
        cc = (cc + npart * nkeep) % sf
        out.append((OutputLayout(nchan, 2 if state == "PPQQ" else 1, nout + 1, 1, 1), 1, nout, nout))
    return out


def all_layouts():
    """every (name, layout, npart, part_step, part_floats) the GPU tests build"""
    for f, call, off, pad, extra in COMPLEX_CASES:
        yield ("complex", f, call, off, pad, extra), *complex_layout(f, off, pad, extra)
    for f, ndim, state, off, pad, pm in DETECT_CASES:
        yield ("detect", f, ndim, off, pad, pm), *detect_layout(f, ndim, off, pad, pm)
    for f, state, sf in SEARCH_CASES:
        for k, lay in enumerate(search_layouts(f, state, sf)):
            yield ("search", f, state, sf, k), *lay
    for f in ("inv_chan", "conv3_14"):                      # a call with fewer parts than the rows have room for, and an empty one
        lay, npart, step, n = complex_layout(f, 2, 1, 2, nparts_room=4)
        yield ("short", f), lay, npart, step, n
        yield ("empty", f), lay, 0, step, n
        lay, _, row, _ = detect_layout(f, 4, 2, 1, False, nparts_room=4)
        yield ("short detect", f), lay, 1, row, row
