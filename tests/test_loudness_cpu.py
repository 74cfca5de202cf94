"""The loudness stage without a GPU: the bindings; xdtts_loudness_filter, _plan and xdtts_true_peak_filter against the fp64
restatement; the rate rule and the argument errors as status codes before a device is touched; the restatement itself against
analytic anchors; the gate margin of every GPU test input; the stand-alone driver of loudness_plan.h under AddressSanitizer
and UBSan."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import loudness_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ("xdtts_loudness_lufs", "xdtts_griffinlim_set_loudness", "xdtts_griffinlim_get_loudness", "xdtts_griffinlim_last_loudness",
       "xdtts_griffinlim_loudness", "xdtts_griffinlim_loudness_batch", "xdtts_loudness_plan", "xdtts_loudness_filter",
       "xdtts_true_peak_filter")


def test_symbols_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "xdtts.h")).read()
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in pkg.SYMBOLS, name
    for attr in ("set_loudness", "get_loudness", "last_loudness", "loudness", "loudness_batch"):
        assert callable(getattr(pkg.GriffinLim, attr))
    assert callable(pkg.loudness_plan) and callable(pkg.loudness_filter) and callable(pkg.true_peak_filter)
    assert C.sizeof(pkg.Loudness) == 40
    assert re.search(r"}\s*xdtts_loudness\s*;", header)


@pytest.mark.parametrize("Q", lr.RATES)
def test_filter_equals_the_restatement(pkg, Q):
    ours, ref = pkg.loudness_filter(Q), lr.coef(Q)
    for (b, a), (rb, ra) in zip(ours, ref):
        assert np.abs(b - rb).max() <= 1e-14 and np.abs(a - ra).max() <= 1e-14 and a[0] == 1.0


def test_filter_is_the_bs1770_table_at_48k(pkg):
    (b1, a1), (b2, a2) = pkg.loudness_filter(48000)
    assert np.abs(b1 - np.array(lr.BS1770_48K[0])).max() <= 1e-12
    assert np.abs(a1[1:] - np.array(lr.BS1770_48K[1])).max() <= 1e-12
    assert np.abs(a2[1:] - np.array(lr.BS1770_48K[2])).max() <= 1e-12
    assert b2.tolist() == [1.0, -2.0, 1.0]


@pytest.mark.parametrize("Q", lr.GPU_RATES)
def test_plan_equals_the_restatement(pkg, Q):
    h = (Q + 5) // 10
    for N in (0, 1, 4 * h - 1, 4 * h, 5 * h - 1, 5 * h, 10 * h + 7):
        assert pkg.loudness_plan(Q, N) == lr.plan(Q, N), (Q, N)
    assert pkg.loudness_plan(11025)["hop"] == 1103
    assert pkg.lib.xdtts_loudness_plan(Q, 5, None, None) == 0  # XDTTS_OK: either out pointer may be NULL


def test_rate_rule(pkg):
    for Q in (7999, 96001, 0, -1):
        assert not lr.supported(Q)
        with pytest.raises(pkg.XdttsError) as e:
            pkg.loudness_plan(Q, 100)
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and str(Q) in str(e.value)
        with pytest.raises(pkg.XdttsError):
            pkg.loudness_filter(Q)
    for Q in (8000, 8001, 22050, 44100, 95999, 96000):
        assert lr.supported(Q) and pkg.loudness_plan(Q)["hop"] == (Q + 5) // 10


def test_argument_errors_come_back_without_a_device(pkg):
    lib, BAD = pkg.lib, pkg.XDTTS_ERR_BAD_ARG
    nan = float("nan")
    # the values first: reported without a handle
    for t, c in ((0.5, nan), (-70.5, nan), (float("inf"), nan), (-16.0, 6.5), (-16.0, -20.5), (nan, float("inf"))):
        assert lib.xdtts_griffinlim_set_loudness(None, t, c) == BAD
        assert b"loudness" in lib.xdtts_last_error()
    assert lib.xdtts_griffinlim_set_loudness(None, -16.0, -1.0) == BAD and b"null" in lib.xdtts_last_error()
    t, c = C.c_float(), C.c_float()
    assert lib.xdtts_griffinlim_get_loudness(None, C.byref(t), C.byref(c)) == BAD
    n = C.c_size_t(7)
    assert lib.xdtts_griffinlim_last_loudness(None, None, 0, C.byref(n)) == BAD and n.value == 0
    x = np.zeros(8, np.float32)
    out = pkg.Loudness()
    assert lib.xdtts_griffinlim_loudness(None, x.ctypes.data, 8, 7999, C.byref(out)) == BAD and b"7999" in lib.xdtts_last_error()
    assert lib.xdtts_griffinlim_loudness(None, x.ctypes.data, 8, 48000, C.byref(out)) == BAD and b"null" in lib.xdtts_last_error()
    assert lib.xdtts_griffinlim_loudness_batch(None, None, None, 0, 48000, None) == BAD
    assert lib.xdtts_loudness_filter(48000, None) == BAD and lib.xdtts_true_peak_filter(None) == BAD
    # the host function: -inf as specified
    assert pkg.Loudness().lufs == -math.inf and lib.xdtts_loudness_lufs(None) == -math.inf
    one = pkg.Loudness(mean_square=1.0)
    assert one.lufs == pytest.approx(-0.691, abs=1e-12)


def test_true_peak_taps_are_the_restatement_rounded_once(pkg):
    t32, t64 = pkg.true_peak_filter(), lr.true_peak_taps()
    assert t32.shape == (3, 24) == t64.shape and t32.dtype == np.float32
    # one fp32 rounding of a double that may differ from numpy's in its last bits (libm sin, the I0 series)
    assert np.all(np.abs(t32.astype(np.float64) - t64) <= 2.0 ** -24 * np.abs(t64) + 1e-14)
    assert np.array_equal(t32[1], t32[1][::-1]) and np.array_equal(t32[0], t32[2][::-1])


# ---- the restatement against analytic anchors -----------------------------------------------------------------------------

def test_full_scale_997_hz_sine_reads_minus_3_01_lufs_at_48k():
    m = lr.measure(lr.sine(48000), 48000)
    assert m["lufs"] == pytest.approx(-3.010, abs=0.001)
    assert m["gated_blocks"] == m["blocks"] == 27


@pytest.mark.parametrize("Q,want", [(22050, -2.981), (8000, -2.996), (11025, -2.969), (96000, -3.028)])
def test_the_sine_at_the_other_rates_reads_what_the_bilinear_shelf_gives(Q, want):
    assert lr.measure(lr.sine(Q), Q)["lufs"] == pytest.approx(want, abs=0.002)


def test_tapered_quarter_rate_burst_reads_0_dbtp():
    tp, sp, _ = lr.true_peak(lr.quarter_rate_burst())
    assert 20 * np.log10(sp) == pytest.approx(-3.01, abs=0.01)
    assert 20 * np.log10(tp) == pytest.approx(0.0, abs=0.01)


def test_transient_gain_of_the_double_pole():
    """kappa enters the tolerance of the GPU tests' mean_square: n eps kappa <= 5e5 2^-53 200 = 1.1e-8."""
    for Q in lr.GPU_RATES:
        assert lr.kappa(Q) <= 200.0, Q
    assert lr.kappa(96000) > lr.kappa(8000)


def test_gain_rule_of_the_restatement():
    m = lr.measure(0.1 * lr.sine(48000), 48000)
    g = lr.gain(m["mean_square"], m["true_peak"], -16.0)
    assert lr.lufs(g * g * m["mean_square"]) == pytest.approx(-16.0, abs=1e-9)
    gc = lr.gain(m["mean_square"], m["true_peak"], -16.0, -20.0)
    assert gc < g and gc * m["true_peak"] == pytest.approx(10 ** (-20.0 / 20), rel=1e-12)
    assert lr.gain(0.0, 0.3, -16.0, -1.0) == 1.0


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Q", lr.GPU_RATES)
def test_gate_margin_of_every_gpu_input(Q):
    """No block of a GPU test input lies within 1e-6 (relative) of a gate threshold: a reassociated fp64 sum cannot move one
    across.  The longest input reaches every branch: blocks only the relative gate removes, blocks the absolute gate removes."""
    for N in sorted(set(lr.lengths(Q)) | set(lr.ragged_lengths(Q))):
        m = lr.measure(lr.speech_like(Q, N), Q)
        assert lr.gate_margin(m) > 1e-6, (Q, N, lr.gate_margin(m))
    m = lr.measure(lr.speech_like(Q, lr.lengths(Q)[-1]), Q)
    assert m["gated_blocks"] < int(m["abs_mask"].sum()) < m["blocks"]


# ---- the stand-alone driver ------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_loudness_plan_driver_under_sanitizers(tmp_path):
    """tests/loudness_plan_test.cpp with plain g++ and -fsanitize=address,undefined: the header's arithmetic and the kernels'
    three-phase scan walked on the host with every index checked."""
    exe = str(tmp_path / "loudness_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "loudness_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "loudness_plan.h"), encoding="utf-8").read()
    assert re.findall(r"#\s*include\s*\"([^\"]+)\"", src) == ["resample_plan.h"]  # of the library's headers, the other plain one
    assert not re.search(r"#\s*include\s*<hip/", src)
