"""The look-ahead true-peak limiter without a device (include/xdtts.h; csrc/limiter_plan.h): the bindings and argument rules, H
and the window against the fp64 restatement (tests/limiter_ref.py), xdtts_limiter_reference against the restatement under an
a-priori bound, the properties of its output, the overshoot of the definition, its effect on the delivered loudness, and the
sanitizer-built stand-alone driver of the plan header."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import limiter_ref as lm
import loudness_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ["xdtts_griffinlim_set_limiter", "xdtts_griffinlim_get_limiter", "xdtts_griffinlim_last_limiter", "xdtts_griffinlim_limit",
       "xdtts_griffinlim_limit_batch", "xdtts_limiter_plan", "xdtts_limiter_window", "xdtts_limiter_reference"]


def test_symbols_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "xdtts.h")).read()
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in pkg.SYMBOLS, name
    for attr in ("set_limiter", "get_limiter", "last_limiter", "limit", "limit_batch"):
        assert callable(getattr(pkg.GriffinLim, attr))
    assert callable(pkg.limiter_plan) and callable(pkg.limiter_window) and callable(pkg.limiter_reference)
    assert C.sizeof(pkg.LimiterStats) == 24 and pkg.LimiterStats.limited.offset == 16
    assert re.search(r"}\s*xdtts_limiter_stats\s*;", header)
    assert C.sizeof(pkg.Loudness) == 40  # xdtts_loudness keeps its layout
    assert "no limiter" not in header


def test_argument_errors_are_status_codes(pkg):
    """before a device is touched: this machine has none"""
    x = np.zeros(10, dtype=np.float32)
    out = np.zeros(10, dtype=np.float32)
    st = pkg.LimiterStats()
    f = pkg.lib.xdtts_limiter_reference
    ok = (x.ctypes.data, 10, 22050, 1.0, 0.5, 5000, out.ctypes.data, C.byref(st))
    assert f(*ok) == 0
    assert f(x.ctypes.data, 10, 22050, 1.0, 0.5, 5000, out.ctypes.data, None) == 0  # stats may be NULL

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return f(*a)

    for i, v in ((1, 0), (1, 1 << 28), (2, 7999), (2, 96001), (3, float("nan")), (3, -1.0), (4, 0.0), (4, -0.5), (4, float("inf")),
                 (5, 0), (5, 499), (5, 10001), (0, None), (6, None)):
        assert with_(i, v) == pkg.XDTTS_ERR_BAD_ARG, (i, v)
    for rate, us in ((7999, 500), (96001, 500), (22050, 0), (22050, 499), (22050, 10001), (22050, -1)):
        assert pkg.lib.xdtts_limiter_plan(rate, us, None, None) == pkg.XDTTS_ERR_BAD_ARG
        assert pkg.lib.xdtts_limiter_window(rate, us, out.ctypes.data) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_limiter_plan(22050, 500, None, None) == 0  # either out pointer may be NULL
    assert pkg.lib.xdtts_limiter_window(22050, 500, None) == pkg.XDTTS_ERR_BAD_ARG
    # the handle entries: the value is looked at before the handle
    assert pkg.lib.xdtts_griffinlim_set_limiter(None, 499) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_set_limiter(None, 500) == pkg.XDTTS_ERR_BAD_ARG  # (null handle)
    assert pkg.lib.xdtts_griffinlim_limit(None, x.ctypes.data, 0, 22050, 1.0, 0.5, 5000, out.ctypes.data, C.byref(st)) == pkg.XDTTS_ERR_BAD_ARG


@pytest.mark.parametrize("Q", lm.RATES)
def test_half_width_equals_the_restatement(pkg, Q):
    for us in (500, 1500, 5000, 10000):
        p = pkg.limiter_plan(Q, us)
        assert p == {"half_width": lm.half_width(Q, us), "tile": lm.TILE}, (Q, us)
        assert 12 <= p["half_width"] <= 960
    assert pkg.limiter_plan(96000, 10000)["half_width"] == 960 and pkg.limiter_plan(8000, 500)["half_width"] == 12


@pytest.mark.parametrize("Q,us", [(8000, 500), (22050, 1500), (22050, 5000), (48000, 10000), (96000, 10000)])
def test_window_equals_the_restatement(pkg, Q, us):
    w = pkg.limiter_window(Q, us)
    ref = lm.window(lm.half_width(Q, us))
    assert np.array_equal(w, ref.astype(np.float32))  # bit for bit
    assert abs(float(ref.sum()) - 1.0) <= 1e-12
    assert np.array_equal(w, w[::-1])


@functools.lru_cache(maxsize=None)
def _case(Q, us, N):
    """(input, the library's reference, its stats, the restatement): computed once, shared, never written to"""
    import importlib

    pkg = importlib.import_module("xd-tts_amd")
    x = lm.signal(Q, us, N)
    x.setflags(write=False)
    out, st = pkg.limiter_reference(x, Q, lm.GAIN0, lm.CEIL, us)
    return x, out, st, lm.limit(x, Q, lm.GAIN0, lm.CEIL, us, w=pkg.limiter_window(Q, us))


@pytest.mark.parametrize("Q", lm.GPU_RATES)
def test_reference_against_fp64(pkg, Q):
    """|out - out64| <= |G x| (B + 3 2^-24) with B = (26 S G max|x| / c + 2 H + 12) 2^-24 (limiter_ref.gain_bound: how it is
    derived); where G x = 0 both are 0.  The recovered gain out / (G x) obeys B itself wherever |G x| is not tiny.  Worst ratios
    to the bound over the 63 shapes: 0.022 (out), recorded in DESIGN.md 4.12."""
    worst = 0.0
    G = float(np.float32(lm.GAIN0))
    for us in lm.LOOKAHEADS:
        for N in lm.lengths(Q, us):
            x, out, st, ref = _case(Q, us, N)
            B = lm.gain_bound(x, Q, lm.GAIN0, lm.CEIL, us)
            err = np.abs(out.astype(np.float64) - ref["out"])
            lim = np.abs(G * x.astype(np.float64)) * (B + 3 * lm.EPS)
            assert np.all(err <= lim), (Q, us, N, float((err / np.maximum(lim, 1e-300)).max()))
            worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()) if np.any(lim > 0) else 0.0)
    print("limiter reference against fp64, rate %d: worst |out - out64| / bound = %.4f" % (Q, worst))


@pytest.mark.parametrize("Q", lm.GPU_RATES)
def test_properties_of_the_reference(pkg, Q):
    """On xdtts_limiter_reference's output: g <= r everywhere (the sample peak of out stays at the ceiling), g = 1 where no r < 1
    lies within 2 H, the stats against the restatement's.  min_gain is a float of the definition's chain: it equals the
    restatement's within the gain bound.  `limited` counts g < 1 in fp32, where a gain closer to 1 than 2^-25 reads as 1: it lies
    between the restatement's count of g < 1 - B and its count of samples within 2 H of a sample that needs a gain (g64 < 1)."""
    G, cf = float(np.float32(lm.GAIN0)), float(np.float32(lm.CEIL))
    for us in lm.LOOKAHEADS:
        H = lm.half_width(Q, us)
        for N in lm.lengths(Q, us):
            x, out, st, ref = _case(Q, us, N)
            x64, o64 = x.astype(np.float64), out.astype(np.float64)
            B = lm.gain_bound(x, Q, lm.GAIN0, lm.CEIL, us)
            assert np.abs(o64).max() <= cf * (1 + 4 * lm.EPS), (Q, us, N)
            # g <= r: |out| <= |G x| r (1 + 2 eps) -- two roundings behind g; r against the restatement's within the gain bound
            assert np.all(np.abs(o64) <= np.abs(G * x64) * (ref["r"] + B) * (1 + 4 * lm.EPS) + 1e-300), (Q, us, N)
            need = ref["r"] < 1.0
            near = lm.sliding_min(np.where(need, 0.0, 1.0), 2 * H)[2 * H:2 * H + N] == 0.0  # some r < 1 within 2 H
            far = ~near
            assert np.array_equal(out[far], (x * np.float32(lm.GAIN0))[far]), (Q, us, N)  # g = 1: the bits of the one-gain scaling
            assert st.half_width == H and st.engaged == 1
            assert abs(st.min_gain - ref["min_gain"]) <= B, (Q, us, N)
            assert int((ref["g"] < 1.0 - B).sum()) <= st.limited <= int(near.sum()), (Q, us, N, st.limited, ref["limited"])


def test_overshoot_of_the_definition():
    """The fp64 true peak (loudness_ref.true_peak) of the restatement's output is at most 0.01 dB above c on every case the CPU
    and GPU tests use.  A property of the definition (the 4x interpolation sees the limited signal, the envelope saw the
    unlimited one): checked on the restatement, never on the device.  Worst recomputed here: 0.0006 dB (the shortest window,
    H = 12)."""
    worst = -np.inf
    cf = float(np.float32(lm.CEIL))
    for Q, us, N in lm.cases():
        ref = _case(Q, us, N)[3]
        tp = lr.true_peak(ref["out"])[0]
        over = 20.0 * np.log10(max(tp, 1e-300) / cf)
        assert over <= 0.01, (Q, us, N, over)
        worst = max(worst, over)
    for Q in (22050, 8000):  # ... and on the signal of the effect test, and on the burst whose peak lies between the samples
        x = lr.speech_like(Q, 3 * Q)
        m = lr.measure(x, Q)
        g0 = lr.gain(m["mean_square"], m["true_peak"], -10.0)
        c = 10.0 ** (-3.0 / 20.0)
        for us in (500, 5000):
            over = 20.0 * np.log10(lr.true_peak(lm.limit(x, Q, g0, c, us)["out"])[0] / float(np.float32(c)))
            assert over <= 0.01, (Q, us, over)
            worst = max(worst, over)
    b = lr.quarter_rate_burst().astype(np.float32)
    ref = lm.limit(b, 48000, 1.0, 0.8, 1500)
    assert np.abs(b).max() * 1.0 < 0.8 and ref["limited"] > 0  # only the interpolated phases are over the ceiling: the stage engages
    over = 20.0 * np.log10(lr.true_peak(ref["out"])[0] / float(np.float32(0.8)))
    assert -0.5 <= over <= 0.01, over  # the result is at the ceiling (e takes a peak between two samples for both: never above, at most a little below)
    print("limiter overshoot of the definition: worst %.4f dB above the ceiling" % max(worst, over))


@pytest.mark.parametrize("Q", (22050, 8000))
def test_effect_on_the_delivered_loudness(Q):
    """speech_like at -10 LUFS under -3 dBTP: the ceiling binds (g0 TP > c), and the restatement's delivered loudness is higher
    than the one-gain rule's."""
    x = lr.speech_like(Q, 3 * Q)
    m = lr.measure(x, Q)
    T, C_db = -10.0, -3.0
    c = 10.0 ** (C_db / 20.0)
    g0 = lr.gain(m["mean_square"], m["true_peak"], T)
    assert g0 * m["true_peak"] > c  # the precondition
    one_gain = lr.measure(x.astype(np.float64) * float(np.float32(lr.gain(m["mean_square"], m["true_peak"], T, C_db))), Q)["lufs"]
    for us in (1500, 5000):
        limited = lr.measure(lm.limit(x, Q, g0, c, us)["out"], Q)["lufs"]
        assert one_gain < limited <= T + 1e-9, (Q, us, one_gain, limited)
        print("limiter effect rate %d, %d us: one gain %.2f LUFS, limiter %.2f LUFS, target %.1f" % (Q, us, one_gain, limited, T))


# ---- the stand-alone driver ------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_limiter_plan_driver_under_sanitizers(tmp_path):
    """tests/limiter_plan_test.cpp with plain g++ and -fsanitize=address,undefined: the rules, and the walk of one tile as a
    workgroup of k_limit performs it, into buffers of the exact size, against the sample-by-sample reference at every shape the
    GPU tests use."""
    exe = str(tmp_path / "limiter_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "limiter_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "limiter_plan.h"), encoding="utf-8").read()
    assert re.findall(r"#\s*include\s*\"([^\"]+)\"", src) == ["loudness_plan.h"]  # of the library's headers, the other plain one
    assert not re.search(r"#\s*include\s*<hip/", src)
