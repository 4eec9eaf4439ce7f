"""CPU restatement of cyclic-spectrum folding (dsp::CyclicFold: the plan, the lag fold and Synch, as include/dspsr_amd.h states
them) for the tests, and the case tables the CPU and GPU tests share.

  rows    complex voltages [nchan][npol_in][ndat] (complex64 / complex128), sample idat of the block at rows[:, :, idat]
  lags    [nbin][npol_out][nchan][nlag] complex: lag[bin][pol][chan][ilag] += x[idat] * conj(y[idat + ilag]),
          bin = plan[ilag % 2][idat + ilag / 2], idat < ndat_fold - nlag (nothing when ndat_fold <= nlag)
  (x, y)  npol_out 1: (p0,p0) then (p1,p1) into one sum; 2: (p0,p0), (p1,p1); 4: + (p0,p1), (p1,p0)

fold(..., dtype=np.float64) is the yardstick; fold(..., dtype=np.float32) keeps every accumulator in float32 and adds the terms
in strict time order, each term formed as the CPU loop forms it (two rounded products, one rounded sum, then the rounded
addition to the accumulator): the reference's own association.
"""
import functools

import numpy as np


def plans(phi, phase_per_sample, nbin, ndat):
    """(plan0, plan1, hits): the double recurrence of the fold plan, evaluated at the sample and half a sample later."""
    p0, p1, hits = np.zeros(ndat, np.int64), np.zeros(ndat, np.int64), np.zeros(nbin, np.uint32)
    phi, pps, dn = float(phi), float(phase_per_sample), float(nbin)
    bps = pps * dn
    for i in range(ndat):
        phi -= np.floor(phi)
        d = phi * dn
        b = int(d)
        phi += pps
        assert b < nbin
        p0[i] = b
        p1[i] = int(d + 0.5 * bps) % nbin
        hits[b] += 1
    return p0, p1, hits


PAIRS = {(1, 1): [(0, 0, 0)], (2, 1): [(0, 0, 0), (0, 1, 1)], (2, 2): [(0, 0, 0), (1, 1, 1)],
         (2, 4): [(0, 0, 0), (1, 1, 1), (2, 0, 1), (3, 1, 0)]}          # (output pol, x pol, y pol)


def _begin(rows, nlag, npol_out, nbin, lags, dtype):
    nchan, _npol_in, _ndat = rows.shape
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    out = np.zeros((nbin, npol_out, nchan, nlag), cdt) if lags is None else lags.astype(cdt).copy()
    return cdt, out


def fold(rows, plan0, plan1, nlag, npol_out, nbin, lags=None, dtype=np.float64):
    """One fold call on the ndat_fold = rows.shape[2] samples of `rows`; returns the lag array (a new one, `lags` + this call).

    The sums of fold_by_sample, bit for bit, in a loop that numpy runs on slices: over u = idat + ilag / 2, where all lags of one
    parity share a bin.  An accumulator (bin, pol, chan, ilag) still receives its terms one at a time in rising idat (u rises
    with idat at a fixed lag) and every term is formed by the same rounded operations, so the association is unchanged;
    tests/test_cyclic_cases_host.py holds the two against each other."""
    nchan, npol_in, ndat = rows.shape
    cdt, out = _begin(rows, nlag, npol_out, nbin, lags, dtype)
    if ndat <= nlag:
        return out
    # channel innermost ([bin][pol][lag][chan] and [pol][sample][chan]): the slices below are then rows of whole channels
    re, im = (np.ascontiguousarray(a.transpose(0, 1, 3, 2)) for a in (out.real, out.imag))
    xr, xi = (np.ascontiguousarray(a.astype(dtype).transpose(1, 2, 0)) for a in (rows.real, rows.imag))
    pl = (np.asarray(plan0), np.asarray(plan1))
    nvalid = ndat - nlag
    for u in range(nvalid + (nlag - 1) // 2):
        for par in (0, 1):
            # lags 2 h + par with idat = u - h in [0, nvalid): h in [h0, h1)
            h0, h1 = max(0, u - nvalid + 1), min((nlag - par + 1) // 2, u + 1)
            if h0 >= h1:
                continue
            b = pl[par][u]
            ix = slice(u - h0, u - h1 if u - h1 >= 0 else None, -1)          # x[u - h]
            iy = slice(u + h0 + par, u + h1 + par)                            # y[u + h + par]
            il = slice(2 * h0 + par, 2 * h1 + par, 2)
            for q, px, py in PAIRS[(npol_in, npol_out)]:
                ar, ai = xr[px, ix], xi[px, ix]
                br, bi = xr[py, iy], xi[py, iy]
                re[b, q, il] = re[b, q, il] + (ar * br + ai * bi)
                im[b, q, il] = im[b, q, il] + (ai * br - ar * bi)
    return (re + 1j * im).astype(cdt).transpose(0, 1, 3, 2).copy()


def fold_by_sample(rows, plan0, plan1, nlag, npol_out, nbin, lags=None, dtype=np.float64):
    """fold() as the CPU engine's loop is written: sample by sample, every lag of the sample at once.  Slow (an indexed update
    of the whole [chan][lag] plane per sample); kept as the statement that fold() is held against."""
    nchan, npol_in, ndat = rows.shape
    cdt, out = _begin(rows, nlag, npol_out, nbin, lags, dtype)
    if ndat <= nlag:
        return out
    re, im = out.real.copy(), out.imag.copy()
    xr, xi = rows.real.astype(dtype), rows.imag.astype(dtype)
    L = np.arange(nlag)
    C = np.arange(nchan)[:, None]
    pl = np.stack([np.asarray(plan0), np.asarray(plan1)])
    for idat in range(ndat - nlag):
        B = pl[L % 2, idat + L // 2][None, :]
        for q, px, py in PAIRS[(npol_in, npol_out)]:
            ar, ai = xr[:, px, idat, None], xi[:, px, idat, None]
            br, bi = xr[:, py, idat:idat + nlag], xi[:, py, idat:idat + nlag]
            re[B, q, C, L] = re[B, q, C, L] + (ar * br + ai * bi)
            im[B, q, C, L] = im[B, q, C, L] + (ai * br - ar * bi)
    return (re + 1j * im).astype(cdt)


def window(nlag, mover):
    """Synch's window on lags l >= 1 for mover > 1, in float as the reference writes it; ones for mover 1."""
    w = np.ones(nlag, np.float32)
    if mover > 1:
        l = np.arange(1, nlag)
        x = (np.pi / 3 * mover * l / float(np.float32(2 * nlag - 2))).astype(np.float32)
        y = (0.5 * (1 + np.cos(2 * np.pi * l.astype(np.float32).astype(np.float64) / float(np.float32(2 * nlag))))).astype(np.float32)
        w[1:] = y * np.sin(x) / x
    return w


def synch(lags, mover):
    """lags [nbin][npol][nchan][nlag] complex -> spectra float64 [nchan * nchan_spec / mover][npol][nbin]: window, unnormalised
    backward complex-to-real transform of nchan_spec = 2 nlag - 2 points, every mover-th point."""
    nbin, npol, nchan, nlag = lags.shape
    n = 2 * nlag - 2
    spec = np.fft.irfft(lags.astype(np.complex128) * window(nlag, mover).astype(np.float64), n, axis=3) * n
    spec = spec[..., ::mover]                                            # [bin][pol][chan][schan]
    return np.ascontiguousarray(spec.transpose(2, 3, 1, 0)).reshape(nchan * (n // mover), npol, nbin)


# ---- exact data: integer real and imaginary parts in [-7, 7]; every |term| <= 7*7 + 7*7 = 98 --------------------------------------
def exact_rows(seed, nchan, npol, ndat):
    rng = np.random.default_rng(seed)
    v = rng.integers(-7, 8, size=(nchan, npol, ndat, 2))
    return (v[..., 0] + 1j * v[..., 1]).astype(np.complex64)


def noise_rows(seed, nchan, npol, ndat, scale):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((nchan, npol, ndat, 2)) * scale
    return (v[..., 0] + 1j * v[..., 1]).astype(np.complex64)


# One case: shape + a list of calls (ndat_fold, idat_start, phi, phase_per_sample, zero_first).  phase_per_sample * nbin is the
# run length's inverse: > 1 gives several bins per sample, << 1 / nlag runs much longer than nlag.
def _case(name, npol_in, npol_out, nlag, nbin, nchan, calls):
    return dict(name=name, npol_in=npol_in, npol_out=npol_out, nlag=nlag, nbin=nbin, nchan=nchan, calls=calls)


EXACT_CASES = [
    _case("nlag2-nbin2", 1, 1, 2, 2, 3, [(2, 0, 0.1, 0.3, False), (3, 0, 0.1, 0.3, False), (1500, 0, 0.95, 0.0004, False)]),
    _case("nlag3-fastbins", 2, 4, 3, 7, 2, [(3, 0, 0.2, 2.3 / 7, False), (4, 5, 0.7, 2.3 / 7, False), (1100, 3, -3.4, 2.3 / 7, False)]),
    _case("nlag33-longruns", 2, 1, 33, 4, 2, [(2000, 0, 5.3, 1.0 / (4 * 700), False), (34, 0, 0.0, 0.01, False)]),
    _case("nlag33-pol2", 2, 2, 33, 1024, 1, [(33, 0, 0.5, 0.01, False), (1200, 7, 0.999, 1.0 / 1024 / 3.7, False)]),
    _case("nlag129-pol4", 2, 4, 129, 64, 3, [(700, 0, 0.3, 1.0 / 64 / 9.3, False), (130, 2, 0.6, 1.0 / 64 / 9.3, False),
                                             (900, 0, 0.1, 1.0 / 64 / 0.4, False)]),
    _case("nlag129-zero", 1, 1, 129, 16, 2, [(600, 0, 0.3, 0.001, False), (1300, 1, 0.4, 0.0007, True)]),
    _case("nlag513", 2, 2, 513, 128, 2, [(513, 0, 0.0, 0.001, False), (514, 0, 0.0, 0.001, False), (1700, 0, 0.25, 1.0 / 128 / 40.5, False)]),
    _case("nlag513-pol1", 1, 1, 513, 5, 1, [(2100, 4, 1.25, 1.0 / 5 / 1900.0, False)]),
    _case("nlag2049-pol4", 2, 4, 2049, 256, 1, [(2049, 0, 0.0, 0.001, False), (2050, 0, 0.9, 0.001, False),
                                                (2049 + 1400, 0, 0.77, 1.0 / 256 / 6.1, False)]),
    _case("nlag2049-pol1", 2, 1, 2049, 32, 2, [(2049 + 700, 6, 0.31, 1.0 / 32 / 333.0, False)]),
]


def check_exact(case):
    """max terms per accumulator x 98 x (2 if npol_out == 1 with two polarisations summed) < 2^24: every partial sum is an
    integer a float32 holds, so every order of summation gives the same bits."""
    terms = sum(max(0, n - case["nlag"]) for n, _, _, _, _ in case["calls"])
    assert terms * 98 * (2 if case["npol_out"] == 1 else 1) < 2 ** 24, case["name"]


@functools.lru_cache(maxsize=None)
def exact_reference(index):
    """(inputs per call, float32 restatement after every call) of EXACT_CASES[index], computed once."""
    case = EXACT_CASES[index]
    check_exact(case)
    lags, steps = None, []
    for k, (ndat, start, phi, pps, zero) in enumerate(case["calls"]):
        rows = exact_rows(1000 * index + k, case["nchan"], case["npol_in"], start + ndat)
        p0, p1, hits = plans(phi, pps, case["nbin"], ndat)
        if zero:
            lags = None
        lags = fold(rows[:, :, start:], p0, p1, case["nlag"], case["npol_out"], case["nbin"], lags, np.float32)
        steps.append((rows, hits, lags))
    return steps


def lag_error(got, ref64):
    """e(X) = max |X - R64| / max |R64| per (chan, pol) lag function; arrays [nbin][npol][nchan][nlag] -> [npol][nchan]"""
    d = np.abs(got.astype(np.complex128) - ref64).max(axis=(0, 3))
    return d / np.abs(ref64).max(axis=(0, 3))
