"""Reference restatements for `dspsr -R`; no device, numpy only, written from the reference's text.

  bandpass_loop      dsp::Bandpass::transformation (Signal/General/Bandpass.C:122-162) with Response::integrate (Response.C:456-492,
                     :587-612 -> cross_detect.ic:37-40): parts in strict time order, numpy.fft, in float64 or float32
  decode_raw         the 8-bit block in the generic order (BitUnpacker.C:48-80) or the CASPSR order (CASPSRUnpacker.C:132-187) as
                     rows [nchan][npol][ndat * ndim], value = (int8 + 0.5) * scale
  median_smooth      fft::median_smooth (PSRCHIVE's; restated: odd window, from the unmodified data, truncated at the edges, element
                     len / 2 of the sorted window)
  rfi_calculate      RFIFilter::calculate (Signal/General/RFIFilter.C:105-162), operation by operation
  rfi_expand         RFIFilter::match (const Response*) (:165-206)
  response_multiply  Response::operator *= (Response.C:73-104, :429-441)
"""
import numpy as np


def bandpass_loop(rows, ndim, resolution, npol_out, dtype=np.float64, out=None, strict=True):
    """rows: [nchan_in][npol_in][>= ndat * ndim] real array of ndat = rows.shape[2] // ndim samples.  Returns
    [npol_out][nchan_in][resolution] of dtype (added to `out` when given).  strict=False adds the parts in one numpy sum instead of
    one by one: for data whose products and sums are exact in any order."""
    dtype = np.dtype(dtype)
    cdtype = np.complex128 if dtype == np.float64 else np.complex64
    rows = np.asarray(rows).astype(dtype)
    nchan_in, npol_in = rows.shape[:2]
    ndat = rows.shape[2] // ndim
    nsamp_fft = resolution if ndim == 2 else 2 * resolution                       # Bandpass.C:78-86
    if ndat < nsamp_fft:
        raise ValueError("error ndat=%d < nfft=%d" % (ndat, nsamp_fft))           # :94-96
    npart = ndat // nsamp_fft                                                     # :99
    if npol_out != npol_in and not (npol_out == 4 and npol_in == 2):
        raise ValueError("npol_out")
    band = np.zeros((npol_out, nchan_in, resolution), dtype=dtype) if out is None else out
    for c in range(nchan_in):
        spec = []
        for p in range(npol_in):
            x = np.ascontiguousarray(rows[c, p, :npart * nsamp_fft * ndim]).reshape(npart, nsamp_fft * ndim)
            if ndim == 1:
                x = np.fft.rfft(x, axis=1)[:, :resolution]                        # frc1d: the Nyquist bin is not kept
            else:
                x = np.fft.fft(x.view(cdtype), axis=1)                            # fcc1d
            assert x.dtype == cdtype
            spec.append(x)
        if not strict:
            if npol_out == 4:
                (pr, pi), (qr, qi) = [(x.real, x.imag) for x in spec]
                for q, v in enumerate((pr * pr + pi * pi, qr * qr + qi * qi, pr * qr + pi * qi, pr * qi - pi * qr)):
                    band[q, c] += v.sum(axis=0)
            else:
                for p in range(npol_in):
                    band[p, c] += (spec[p].real * spec[p].real + spec[p].imag * spec[p].imag).sum(axis=0)
            continue
        for ipart in range(npart):                                                # strict time order
            if npol_out == 4:
                (pr, pi), (qr, qi) = [(s[ipart].real, s[ipart].imag) for s in spec]
                band[0, c] += pr * pr + pi * pi                                   # cross_detect.ic:37-40
                band[1, c] += qr * qr + qi * qi
                band[2, c] += pr * qr + pi * qi
                band[3, c] += pr * qi - pi * qr
            else:
                for p in range(npol_in):
                    re, im = spec[p][ipart].real, spec[p][ipart].imag
                    band[p, c] += re * re + im * im                               # Response.C:484-489
    return band


def encode_raw(values, layout):
    """int8 codes [nchan][npol][ndat][ndim] -> the byte block (uint8, one-dimensional).  layout "generic" or "caspsr"."""
    v = np.asarray(values).astype(np.int8)
    nchan, npol, ndat, ndim = v.shape
    if layout == "generic":
        return np.ascontiguousarray(v.transpose(2, 0, 1, 3)).reshape(-1).view(np.uint8)
    assert (nchan, npol, ndim) == (1, 2, 1) and ndat % 4 == 0
    return np.ascontiguousarray(v[0, :, :, 0].reshape(2, ndat // 4, 4).transpose(1, 0, 2)).reshape(-1).view(np.uint8)


def decode_raw(raw, layout, nchan, npol, ndim, scale, dtype=np.float64):
    """the byte block -> rows [nchan][npol][ndat * ndim], (int8 + 0.5) * scale"""
    b = np.asarray(raw).view(np.int8)
    if layout == "generic":
        ndat = b.size // (nchan * npol * ndim)
        v = b[:ndat * nchan * npol * ndim].reshape(ndat, nchan, npol, ndim).transpose(1, 2, 0, 3)
    else:
        assert (nchan, npol, ndim) == (1, 2, 1)
        ngroup = b.size // 8
        v = b[:ngroup * 8].reshape(ngroup, 2, 4).transpose(1, 0, 2).reshape(1, 2, ngroup * 4, 1)
    return ((v.astype(np.float64) + 0.5) * scale).astype(dtype).reshape(nchan, npol, -1)


def median_smooth(data, wsize):
    data = np.asarray(data)
    if wsize % 2 == 0:
        wsize += 1
    n, h = data.size, wsize // 2
    out = np.empty_like(data)
    for i in range(n):
        win = np.sort(data[max(0, i - h):min(n - 1, i + h) + 1])
        out[i] = win[win.size // 2]
    return out


def rfi_calculate(p0, p1, median_window=51, keep_zapped=True, dtype=np.float32):
    """RFIFilter.C:105-162.  dtype float32 is the reference's arithmetic (float spectrum, double variance, float cutoff); float64
    carries everything in double.  Returns a dict: mask, p0, p1 (zeroed where zapped), total_zapped, rounds, cutoffs, endless (a round
    of re-zaps only: the reference's loop would repeat it for ever; the state is that round's), margin (the smallest relative
    distance of any evaluated statistic from its cutoff, or of a neighbour difference from 2 * cutoff, over all rounds)."""
    T = np.dtype(dtype).type
    p0 = np.array(p0, dtype=dtype).ravel()
    p1 = np.array(p1, dtype=dtype).ravel()
    n = p0.size
    spectrum = p0 + p1                                                            # :116-117
    smooth = median_smooth(spectrum, median_window)                               # :119
    spectrum = smooth - (p0 + p1)                                                 # :124
    spectrum = spectrum * spectrum                                                # :125
    variance = 0.0
    for v in spectrum:                                                            # :127, a double sum in channel order
        variance += float(v)
    variance /= n                                                                 # :130
    mask = np.ones(n, dtype=dtype)
    ever = np.zeros(n, dtype=bool)
    spectrum = list(spectrum)
    zapped, rounds, total, cutoffs, endless, margin = True, 0, 0, [], False, np.inf
    fn = T(n)
    while zapped:                                                                 # :139-158
        cutoff = T(16.0 * variance)                                               # :141
        cutoffs.append(cutoff)
        zapped, fresh = False, False
        rounds += 1
        two = T(2) * cutoff
        for i in range(n):
            s = spectrum[i]
            d = abs(s - spectrum[i - 1]) if i else None
            if cutoff != 0:
                margin = min(margin, abs(float(s) - float(cutoff)) / abs(float(cutoff)))
                if i:
                    margin = min(margin, abs(float(d) - float(two)) / abs(float(two)))
            if s > cutoff or (i and d > two):                                     # :148-149
                variance -= float(s / fn)                                         # :150
                spectrum[i] = T(0)
                p0[i] = p1[i] = mask[i] = 0                                       # :151
                total += 1
                zapped = True
                fresh = fresh or not ever[i]
                ever[i] = True
            elif not (keep_zapped and ever[i]):
                mask[i] = 1                                                       # :156
        if zapped and not fresh:
            endless = True
            break
    return {"mask": mask, "p0": p0, "p1": p1, "total_zapped": total, "rounds": rounds, "cutoffs": np.array(cutoffs, dtype=dtype),
            "endless": endless, "margin": margin}


def rfi_expand(mask, required):
    """RFIFilter.C:180-196: complex64 [required]"""
    mask = np.asarray(mask, dtype=np.float32)
    n = mask.size
    expand, shrink = required // n, (n // required if required else 0)
    ph = np.ones(required, dtype=np.complex64)
    if expand:
        for ip in range(expand):
            ph[ip:n * expand:expand] = mask
    elif shrink:
        for idat in range(required):
            for ip in range(expand):                                              # expand == 0: never runs
                if mask[idat * shrink + ip] == 0.0:
                    ph[idat] = 0.0
    return ph


def response_multiply(kernel, phasors):
    """Response.C:431-437 in float32, one rounding per product and per sum"""
    k = np.asarray(kernel, dtype=np.complex64)
    f = np.asarray(phasors, dtype=np.complex64)
    d_r, d_i, f_r, f_i = k.real.copy(), k.imag.copy(), f.real.copy(), f.imag.copy()
    out = np.empty(k.shape, dtype=np.complex64)
    out.real = f_r * d_r - f_i * d_i
    out.imag = f_i * d_r + f_r * d_i
    return out
