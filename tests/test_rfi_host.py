"""The host code of `dspsr -R` (csrc/host_prep.cpp: RFIFilter::calculate, RFIFilter::match(const Response*), Response::operator *=)
bit for bit against the numpy restatement written from the reference's text (tests/rfi_reference.py), through the library and
through a stand-alone driver built with the address and undefined-behaviour sanitizers (nothing is loaded into Python there).  CPU only.

Of the issue's cases, "a channel re-zapped through its neighbour" is NOT here: it cannot be reached (below), and the `rezap` case
stands in its place.

A note on two of the cases.  In RFIFilter.C:148-149 the statistic of every channel is a square and the cutoff is 16 x their mean, so as
long as the cutoff is not negative a channel whose neighbour difference exceeds 2 x cutoff exceeds the cutoff itself (its left
neighbour is either zeroed or at most the cutoff): the neighbour test never decides alone, and a zeroed channel never triggers again.
The `step` case exercises the clause all the same.  A channel is re-zapped only with a cutoff below zero -- `variance -= s / n` in
float against a double mean can leave one -- and then every zeroed channel triggers in every round and the reference's loop does not
end: the `rezap` case (n = 1000, where s / n rounds) checks that the library and the restatement count the same re-zaps and both stop
at the first round that zaps nothing new."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rfi_reference as rr
from dspsr_amd import DspsrAmdError, rfi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024


def _noise(seed=3):
    rng = np.random.default_rng(seed)
    return rng.gamma(1e4, 1.0, N).astype(np.float32), rng.gamma(1e4, 1.0, N).astype(np.float32)    # 10^4 summed |X|^2 per channel


def _tones():
    p0, p1 = _noise()
    for first, width in ((0, 1), (1, 2), (511, 5), (1023, 1), (300, 1), (700, 2)):
        p0[first:first + width] += 3e3 * (1 + first % 3)
        p1[first:first + width] += 2e3
    return p0, p1


def _step():
    p0, p1 = _noise(5)
    p0[600:] *= 2
    p1[600:] *= 2
    p0[100] += 5e3
    return p0, p1


def _weak():
    p0, p1 = _noise(7)
    p0[200] += 4e4                 # alone it sets a cutoff far above the weak tone's statistic
    p0[640] += 2.5e3               # caught once the strong tone has left the variance
    return p0, p1


def _rezap():
    """n = 1000: a flat passband with one tone whose s / 1000 in float lies above s / 1000 in double"""
    n = 1000
    for k in range(1, 200):
        p0 = np.full(n, 100.0, np.float32)
        p0[10] += np.float32(k)
        s = np.float32(np.float32(2 * k) * np.float32(2 * k))             # spectrum = (p0 + p1 - median)^2 with p1 = p0
        if float(s / np.float32(n)) > float(s) / n:
            return p0, p0.copy()
    raise AssertionError("no such tone")


CASES = {"equal": lambda: (np.full(N, 7.0, np.float32), np.full(N, 9.0, np.float32)), "noise": _noise, "tones": _tones, "step": _step,
         "weak": _weak, "rezap": _rezap}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    assert got["total_zapped"] == want["total_zapped"] and got["rounds"] == want["rounds"]
    for key in ("mask", "p0", "p1", "cutoffs"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key


def _library(p0, p1, window, keep):
    try:
        return rfi.mask_calculate(p0, p1, window, keep), False
    except DspsrAmdError as e:
        assert "does not end" in str(e)
        return None, True


@pytest.mark.parametrize("keep", [True, False], ids=["keep", "literal"])
@pytest.mark.parametrize("name", [k for k in CASES if k != "rezap"])
def test_calculate_matches_the_restatement(name, keep):
    p0, p1 = CASES[name]()
    want = rr.rfi_calculate(p0, p1, 51, keep)
    got, endless = _library(p0, p1, 51, keep)
    assert not endless and not want["endless"]
    _same(got, want)
    if not keep:                                            # the literal loop: all ones, only the zeros in p0 / p1 survive
        assert np.all(got["mask"] == 1)
    kept = rr.rfi_calculate(p0, p1, 51, True)
    assert np.array_equal(got["p0"] == 0, kept["mask"] == 0) and np.array_equal(got["p1"] == 0, kept["mask"] == 0)


def test_what_the_cases_exercise():
    eq = rr.rfi_calculate(*CASES["equal"]())
    assert eq["total_zapped"] == 0 and eq["rounds"] == 1 and eq["cutoffs"][0] == 0
    assert rr.rfi_calculate(*_noise())["total_zapped"] == 0
    t = rr.rfi_calculate(*_tones())
    zapped = np.flatnonzero(t["mask"] == 0)
    assert set(zapped) == {0, 1, 2, 511, 512, 513, 514, 515, 1023, 300, 700, 701}
    w = rr.rfi_calculate(*_weak())
    assert w["rounds"] == 3 and set(np.flatnonzero(w["mask"] == 0)) == {200, 640}
    first = rr.rfi_calculate(*_weak())["cutoffs"]
    assert first[1] < first[0]                              # the variance dropped: 640 is caught in round 2 only
    s = rr.rfi_calculate(*_step())
    assert 100 in np.flatnonzero(s["mask"] == 0)
    # an even window is made odd
    assert np.array_equal(rr.median_smooth(np.arange(9.0), 4), rr.median_smooth(np.arange(9.0), 5))
    assert np.array_equal(rr.median_smooth(np.array([5.0, 1, 4, 2, 3]), 3), [5, 4, 2, 3, 3])


def test_a_negative_cutoff_re_zaps_and_is_stopped():
    p0, p1 = _rezap()
    want = rr.rfi_calculate(p0, p1, 51, True)
    assert want["endless"] and want["cutoffs"][1] < 0 and want["total_zapped"] == 1 + 1000 + 1000 and want["rounds"] == 3
    got, endless = _library(p0, p1, 51, True)
    assert endless and got is None                          # the wrapper raises by default ...
    for keep in (True, False):                              # ... and on request hands back the state of the stopping round
        got = rfi.mask_calculate(p0, p1, 51, keep, allow_endless=True)
        assert got["endless"]
        _same(got, rr.rfi_calculate(p0, p1, 51, keep))
    assert not rfi.mask_calculate(*_tones(), allow_endless=True)["endless"]


def test_float32_and_float64_restatements_agree_on_the_cases():
    for name in ("noise", "tones", "weak"):
        p0, p1 = CASES[name]()
        assert np.array_equal(rr.rfi_calculate(p0, p1, 51, True, np.float64)["mask"], rr.rfi_calculate(p0, p1, 51, True)["mask"])


@pytest.mark.parametrize("required", [512, 1024, 4096, 3 * 1024 + 7])
def test_expand(required):
    mask = rr.rfi_calculate(*_tones())["mask"]
    want = rr.rfi_expand(mask, required)
    got = rfi.mask_expand(mask, required)
    assert got.dtype == np.complex64 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if required == 512:
        assert np.all(got == 1)                             # the shrink loop never runs
    if required == 4096:
        assert np.array_equal(got.real.reshape(1024, 4), np.repeat(mask[:, None], 4, axis=1))
    if required == 3 * 1024 + 7:
        assert np.all(got[3 * 1024:] == 1) and np.array_equal(got.real[:3072:3], mask)
    assert not got.imag.any()


def test_response_multiply():
    rng = np.random.default_rng(1)
    kernel = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex64)
    ones = np.ones(4096, np.complex64)
    assert np.array_equal(rfi.response_multiply(kernel, ones).view(np.uint32), kernel.view(np.uint32))      # untouched, bit for bit
    ph = rr.rfi_expand(rr.rfi_calculate(*_tones())["mask"], 4096)
    got = rfi.response_multiply(kernel, ph)
    assert np.array_equal(got.view(np.uint32), rr.response_multiply(kernel, ph).view(np.uint32))
    assert np.all(got[ph == 0] == 0) and np.array_equal(got[ph == 1], kernel[ph == 1])
    general = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex64)
    assert np.array_equal(rfi.response_multiply(kernel, general).view(np.uint32), rr.response_multiply(kernel, general).view(np.uint32))
    with pytest.raises(DspsrAmdError, match="ndat\\*nchan"):
        rfi.response_multiply(kernel, ones[:5])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rfi") / "rfi_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "rfi_driver.cpp"),
           os.path.join(ROOT, "dspsr_amd", "csrc", "host_prep.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_the_cases_through_the_sanitized_driver(driver, tmp_path):
    """the same cases, expands and products through an executable with its own main, built with -fsanitize=address,undefined"""
    rec, expect = [], []
    for name, make in CASES.items():
        for keep in (1, 0):
            p0, p1 = make()
            rec.append(struct.pack("<4I", 1, p0.size, 51, keep) + p0.tobytes() + p1.tobytes())
            expect.append(("calc", p0.size, rr.rfi_calculate(p0, p1, 51, bool(keep))))
    mask = rr.rfi_calculate(*_tones())["mask"]
    for required in (512, 1024, 4096, 3 * 1024 + 7):
        rec.append(struct.pack("<2IQ", 2, mask.size, required) + mask.tobytes())
        expect.append(("expand", required, rr.rfi_expand(mask, required)))
    rng = np.random.default_rng(2)
    kernel = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex64)
    for ph in (np.ones(4096, np.complex64), rr.rfi_expand(mask, 4096)):
        rec.append(struct.pack("<IQ", 3, kernel.size) + kernel.tobytes() + ph.tobytes())
        expect.append(("mul", kernel.size, rr.response_multiply(kernel, ph)))
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(rec))
    p = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = dst.read_bytes()
    pos = 0

    def take(dtype, count):
        nonlocal pos
        a = np.frombuffer(out, dtype=dtype, count=count, offset=pos)
        pos += a.nbytes
        return a

    for kind, n, want in expect:
        rc = int(take(np.int32, 1)[0])
        if kind == "calc":
            total, rounds = (int(v) for v in take(np.uint32, 2))
            mask_, p0_, p1_, cut = take(np.uint32, n), take(np.uint32, n), take(np.uint32, n), take(np.uint32, n + 2)
            assert rc == (-4 if want["endless"] else 0)
            assert (total, rounds) == (want["total_zapped"], want["rounds"])
            assert np.array_equal(mask_, _bits(want["mask"])) and np.array_equal(p0_, _bits(want["p0"])) and np.array_equal(p1_, _bits(want["p1"]))
            assert np.array_equal(cut[:rounds], _bits(want["cutoffs"]))
        else:
            assert rc == 0
            assert np.array_equal(take(np.uint32, 2 * n), want.view(np.uint32))
    assert pos == len(out)
