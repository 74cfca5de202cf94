"""The output-rate stage without a GPU: the bindings; xdtts_resample_plan against the restatement; the rate rule; the library's
own fp32 taps (xdtts_resample_filter) against the fp64 restatement and against the filter figures of include/xdtts.h; the
restatement against scipy; argument errors as status codes before a device is touched; the stand-alone driver of
resample_plan.h under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ("xdtts_griffinlim_set_output_rate", "xdtts_griffinlim_get_output_rate", "xdtts_resample_plan", "xdtts_resample_filter",
       "xdtts_griffinlim_resample", "xdtts_griffinlim_resample_batch")


def test_symbols_are_declared_exported_bound_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "xdtts.h")).read()
    mirror = open(os.path.join(ROOT, "include", "xdtts_host.hpp")).read()
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in pkg.SYMBOLS, name
        assert name in mirror, name
    for attr in ("set_output_rate", "get_output_rate", "resample", "resample_batch"):
        assert callable(getattr(pkg.GriffinLim, attr))
    assert callable(pkg.resample_plan) and callable(pkg.resample_filter)


@pytest.mark.parametrize("Q", rr.RATES)
def test_plan_equals_the_restatement(pkg, Q):
    for N in (0, 1, 2, 255, 256, 885, 4097, 204544, 2 ** 30):
        assert pkg.resample_plan(Q, N) == rr.plan(Q, N), (Q, N)
    # any out pointer may be NULL
    n = C.c_size_t()
    assert pkg.lib.xdtts_resample_plan(Q, 885, None, None, None, C.byref(n)) == 0 and n.value == rr.plan(Q, 885)["n_out"]
    assert pkg.lib.xdtts_resample_plan(Q, 885, None, None, None, None) == 0


def test_rate_rule(pkg):
    for Q in (7999, 96001, 22051, 0, -1):
        assert not rr.supported(Q)
        with pytest.raises(pkg.XdttsError) as e:
            pkg.resample_plan(Q, 100)
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
        assert str(Q) in str(e.value) and ("640" in str(e.value) or "8000" in str(e.value))  # the rate and the rule
        with pytest.raises(pkg.XdttsError) as e:
            pkg.resample_filter(Q)
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
        # the option and the hooks refuse it before any handle or device is looked at
        assert pkg.lib.xdtts_griffinlim_set_output_rate(None, Q) == pkg.XDTTS_ERR_BAD_ARG
        assert str(Q).encode() in pkg.lib.xdtts_last_error()
        assert pkg.lib.xdtts_griffinlim_resample(None, None, 0, Q, None, None) == pkg.XDTTS_ERR_BAD_ARG
        assert str(Q).encode() in pkg.lib.xdtts_last_error()
    # 22050 is the identity: no filter, N' = N
    assert pkg.resample_plan(22050, 12345) == {"L": 1, "M": 1, "half_len": 0, "n_out": 12345}
    assert pkg.resample_filter(22050).tolist() == [1.0]
    for Q in rr.RATES + (22050, 8820, 9600, 14700):
        assert rr.supported(Q)
        pkg.resample_plan(Q, 1)


def test_argument_errors_come_back_without_a_device(pkg):
    x = np.zeros(8, np.float32)
    out = np.zeros(64, np.float32)
    n = C.c_size_t(7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert pkg.lib.xdtts_griffinlim_resample(None, ptr(x), 8, 8000, ptr(out), C.byref(n)) == pkg.XDTTS_ERR_BAD_ARG and n.value == 0
    assert b"null" in pkg.lib.xdtts_last_error()
    assert pkg.lib.xdtts_griffinlim_resample_batch(None, None, None, 0, 8000, None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_get_output_rate(None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_set_output_rate(None, 8000) == pkg.XDTTS_ERR_BAD_ARG and b"null" in pkg.lib.xdtts_last_error()
    # the filter: the size alone, and a buffer that is too small
    assert pkg.lib.xdtts_resample_filter(11025, None, 0, C.byref(n)) == 0 and n.value == 129
    assert pkg.lib.xdtts_resample_filter(11025, ptr(out), 64, C.byref(n)) == pkg.XDTTS_ERR_BAD_ARG


@pytest.fixture(scope="module")
def filters(pkg):
    """(the library's fp32 taps, the restatement's fp64 taps) per rate, computed once."""
    return {Q: (pkg.resample_filter(Q), rr.taps(Q)) for Q in rr.RATES}


@pytest.mark.parametrize("Q", rr.RATES)
def test_taps_are_the_restatement_rounded_once(filters, Q):
    h32, h64 = filters[Q]
    H = rr.plan(Q)["half_len"]
    assert h32.dtype == np.float32 and h32.size == 2 * H + 1 == h64.size
    assert 129 <= h32.size <= 40961
    want = h64.astype(np.float32)
    # within one fp32 ulp, tap by tap: a few double ulps of libm difference move the single rounding by at most one step
    step = np.maximum(np.abs(np.nextafter(want, np.float32(np.inf)) - want), np.abs(want - np.nextafter(want, np.float32(-np.inf))))
    assert np.all(np.abs(h32.astype(np.float64) - want.astype(np.float64)) <= step.astype(np.float64))
    assert np.count_nonzero(h32 != want) <= h32.size // 100  # and nearly all of them are the same float
    assert np.array_equal(h32, h32[::-1])  # exactly symmetric


def response_db(h, L, W, nfft=1 << 21):
    """(f in units of the lower rate's Nyquist, 20 log10 |H(f)| / L) of the taps at the interpolated rate L R."""
    Hf = np.abs(np.fft.rfft(np.asarray(h, dtype=np.float64), nfft)) / L
    f = np.arange(Hf.size) / nfft * (2.0 * W)  # the lower Nyquist is 1 / (2 W) cycles per sample of the interpolated rate
    return f, 20.0 * np.log10(np.maximum(Hf, 1e-300))


@pytest.mark.parametrize("Q", rr.RATES)
def test_the_librarys_own_taps_meet_the_filter_figures(filters, Q):
    h32, _ = filters[Q]
    p = rr.plan(Q)
    L, W = p["L"], max(p["L"], p["M"])
    f, db = response_db(h32, L, W)
    ripple = np.max(np.abs(db[f <= 0.8]))
    stop = np.max(db[f >= 1.0])
    dc = np.array([h32[r::L].astype(np.float64).sum() for r in range(L)])  # (each slice is one residue class of k mod L)
    print("rate %d: passband ripple %.6f dB, stopband %.2f dB, phase DC gain within %.2e of 1" % (Q, ripple, stop, np.max(np.abs(dc - 1.0))))
    assert ripple <= 0.001
    assert stop <= -99.0
    assert np.max(np.abs(dc - 1.0)) <= 1e-5
    taps_per_output = int(np.ceil(h32.size / L))
    assert 65 <= taps_per_output <= 177


def test_restatement_equals_scipy():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.Generator(np.random.PCG64(3))
    for Q in rr.RATES:
        p = rr.plan(Q)
        h = rr.taps(Q)
        for N in (1, 2, 255, 885, 4097):
            x = rng.uniform(-1.0, 1.0, N)
            y, c, a = rr.convolve(x, h, Q)
            want = signal.resample_poly(x, p["L"], p["M"], window=h / p["L"])
            assert y.size == want.size == rr.plan(Q, N)["n_out"], (Q, N)
            assert np.max(np.abs(y - want)) <= 1e-12, (Q, N)
            assert c.max() <= 177 and np.all(a >= np.abs(y) - 1e-15)


def test_restatement_is_zero_phase_and_transparent_in_the_passband():
    """y[0] sits on x[0]: a 1 kHz sine keeps amplitude and phase at the new rate, away from the ends."""
    t = np.arange(8192) / 22050.0
    x = np.sin(2 * np.pi * 1000.0 * t + 0.3)
    for Q in (8000, 48000):
        y, _, _ = rr.convolve(x, rr.taps(Q), Q)
        p = rr.plan(Q)
        edge = p["half_len"] // p["M"] + 1
        m = np.arange(y.size)[edge:-edge]
        assert np.max(np.abs(y[edge:-edge] - np.sin(2 * np.pi * 1000.0 * m / Q + 0.3))) < 2e-5


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_resample_plan_driver_under_sanitizers(tmp_path):
    """tests/resample_plan_test.cpp with plain g++ and -fsanitize=address,undefined: the header's arithmetic and the kernel's walk
    over the table with every index checked."""
    exe = str(tmp_path / "resample_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "resample_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "resample_plan.h"), encoding="utf-8").read()
    assert not re.search(r"#\s*include\s*\"", src)  # none of the library's headers
    assert not re.search(r"#\s*include\s*<hip/", src)
