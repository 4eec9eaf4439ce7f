"""The input of the `dspsr -R` pipeline tests (tests/test_gpu_rfi_pipeline.py), built without a device so that the host suite can
check the condition its comparisons rest on (tests/test_rfi_pipeline_host.py): 8-bit CASPSR-layout noise with the synthetic pulsar
of dspsr_amd.synth plus two continuous tones placed on forward-transform bins of the 1024-channel passband."""
import functools

import numpy as np

import matrix_cases as mc
import rfi_reference as rr
import dspsr_amd
from dspsr_amd import synth

FREQ, BW, TSAMP, DM, PERIOD, NCHAN, FREQ_RES, NBIN = 1382.0, -16.0, 1.0 / 32.0, 3.0, 0.004, 16, 256, 64
PARTS, NBLOCK = 3, 3
NCHAN_BP, WINDOW, BLOCK = 1024, 51, 8192
INTERVAL = 7.5 * BLOCK * TSAMP * 1e-6           # seconds: the loop of RFIFilter.C:91-95 reads eight 8192-sample blocks
TONES = ((100, 10.0, 8.0, 0.3), (700, 7.0, 9.0, 1.1))      # (bin of the 2048-sample transform, amplitude pol 0, pol 1, phase)
SEED = 20100413


def response():
    r = dspsr_amd.Dedispersion(FREQ, BW, DM)
    r.set_frequency_resolution(FREQ_RES)
    return r.match(NCHAN)


def plan(o):
    r = response()
    return mc.make_plan(o, NCHAN, FREQ_RES, (r.impulse_pos, r.impulse_neg), True)


@functools.lru_cache(maxsize=None)
def stream(nsamp_step, nsamp_overlap, seed=SEED):
    """the CASPSR-ordered bytes (int8, one-dimensional) of NBLOCK * PARTS parts"""
    ndat = NBLOCK * PARTS * nsamp_step + nsamp_overlap
    assert ndat % 4 == 0 and ndat >= blocks_used() * BLOCK
    q = synth.voltages(ndat, FREQ, BW, TSAMP, DM, PERIOD, seed=seed).reshape(ndat, 2).astype(np.int64)
    t = np.arange(ndat)
    for k, a0, a1, ph in TONES:
        c = np.cos(2 * np.pi * k * t / (2.0 * NCHAN_BP) + ph)
        q[:, 0] += np.rint(a0 * c).astype(np.int64)
        q[:, 1] += np.rint(a1 * c).astype(np.int64)
    q = np.clip(q, -128, 127).astype(np.int8)
    return np.ascontiguousarray(q.reshape(ndat // 4, 4, 2).transpose(0, 2, 1)).reshape(-1)


def blocks_used():
    """RFIFilter.C:91-95 with Bandpass.C:164: blocks read until integration_length >= interval"""
    rate = 1e6 / TSAMP
    n, length = 0, 0.0
    while length < INTERVAL:
        n += 1
        length += float(BLOCK) / rate
    return n


def restatement(raw, dtype=np.float32, keep_zapped=True):
    """the passband of the first blocks_used() blocks and RFIFilter::calculate on it, both in `dtype`"""
    scale = dspsr_amd.eight_bit_scale()
    rows = rr.decode_raw(raw, "caspsr", 1, 2, 1, 1.0, np.float32)                # int8 + 0.5, exact
    rows = (rows * np.float32(scale)).astype(np.float32)                         # what the unpacker hands on
    used = blocks_used() * BLOCK
    band = rr.bandpass_loop(rows[:, :, :used], 1, NCHAN_BP, 2, dtype)
    return band, rr.rfi_calculate(band[0, 0], band[1, 0], WINDOW, keep_zapped, dtype)
