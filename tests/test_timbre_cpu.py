"""The timbre stage without a device (include/xdtts.h; csrc/timbre_plan.h): the bindings, the struct and the argument rules, the
properties of the fp64 restatement (tests/timbre_ref.py) -- the pitch stays under vtl, the harmonics give way under breath, a
formant moves to b / vtl -- the fp32 yardstick, the breath noise against the library's host function bit for bit, and the
sanitizer-built stand-alone driver of the plan header."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import timbre_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ["xdtts_timbre_default", "xdtts_griffinlim_set_timbre", "xdtts_griffinlim_get_timbre", "xdtts_griffinlim_timbre_linear",
       "xdtts_griffinlim_timbre_linear_batch", "xdtts_timbre_noise_bits"]


def test_symbols_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "xdtts.h")).read()
    host = open(os.path.join(ROOT, "include", "xdtts_host.hpp")).read()
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in pkg.SYMBOLS, name
    for name in NEW[:5]:  # the C++ mirror wraps the handle's entries and the default
        assert re.search(r"\b%s\s*\(" % name, host), name
    for attr in ("set_timbre", "get_timbre", "timbre_linear", "timbre_linear_batch"):
        assert callable(getattr(pkg.GriffinLim, attr))
    assert callable(pkg.timbre_noise_bits)
    assert re.search(r"}\s*xdtts_timbre\s*;", header)


def test_struct_and_default(pkg):
    assert C.sizeof(pkg.Timbre) == 20
    assert [f[0] for f in pkg.Timbre._fields_] == ["vtl", "breath", "seed", "lifter", "log_floor"]
    assert (pkg.Timbre.vtl.offset, pkg.Timbre.breath.offset, pkg.Timbre.seed.offset, pkg.Timbre.lifter.offset, pkg.Timbre.log_floor.offset) == (0, 4, 8, 12, 16)
    t = pkg.Timbre()
    assert t.astuple() == (1.0, 0.0, 1, 30, float(np.float32(1e-5)))
    pkg.lib.xdtts_timbre_default(None)  # a null pointer is ignored


def test_argument_errors_are_status_codes(pkg):
    """The fields are looked at before the handle: with a null handle a bad field is reported by name, a good setting as the null
    handle -- and this machine has no device to touch."""
    S = np.ones((513, 2), dtype=np.float32)
    out = np.empty_like(S)
    bad = (("vtl", 0.49), ("vtl", 2.01), ("vtl", float("nan")), ("vtl", float("inf")), ("breath", -0.01), ("breath", 1.01),
           ("breath", float("nan")), ("breath", float("-inf")), ("lifter", 0), ("lifter", 256), ("log_floor", 0.0), ("log_floor", -1e-5),
           ("log_floor", float("nan")), ("log_floor", float("inf")))
    for field, v in bad:
        t = pkg.Timbre(**{field: v})
        for st in (pkg.lib.xdtts_griffinlim_set_timbre(None, C.byref(t)),
                   pkg.lib.xdtts_griffinlim_timbre_linear(None, S.ctypes.data, 2, C.byref(t), out.ctypes.data)):
            assert st == pkg.XDTTS_ERR_BAD_ARG, (field, v)
            assert field in pkg.lib.xdtts_last_error().decode(), (field, v, pkg.lib.xdtts_last_error())
    good = pkg.Timbre(vtl=1.25, breath=0.5)
    assert pkg.lib.xdtts_griffinlim_set_timbre(None, C.byref(good)) == pkg.XDTTS_ERR_BAD_ARG
    assert "handle" in pkg.lib.xdtts_last_error().decode()
    assert pkg.lib.xdtts_griffinlim_set_timbre(None, None) == pkg.XDTTS_ERR_BAD_ARG  # (NULL = the default: the null handle is what fails)
    assert "handle" in pkg.lib.xdtts_last_error().decode()
    assert pkg.lib.xdtts_griffinlim_get_timbre(None, C.byref(good)) == pkg.XDTTS_ERR_BAD_ARG
    # the frame count of the stage alone: 1 .. 2^20, before the handle
    for n in (0, (1 << 20) + 1):
        assert pkg.lib.xdtts_griffinlim_timbre_linear(None, S.ctypes.data, n, C.byref(good), out.ctypes.data) == pkg.XDTTS_ERR_BAD_ARG
        assert "frames" in pkg.lib.xdtts_last_error().decode()
    # the ragged form names the utterance
    ta = (pkg.Timbre * 3)(pkg.Timbre(), pkg.Timbre(vtl=1.5), pkg.Timbre(breath=2.0))
    sp = (C.c_void_p * 3)(*[S.ctypes.data] * 3)
    op = (C.c_void_p * 3)(*[out.ctypes.data] * 3)
    nf = (C.c_size_t * 3)(2, 2, 2)
    assert pkg.lib.xdtts_griffinlim_timbre_linear_batch(None, sp, nf, 3, ta, op) == pkg.XDTTS_ERR_BAD_ARG
    msg = pkg.lib.xdtts_last_error().decode()
    assert "utterance 2" in msg and "breath" in msg, msg
    assert pkg.lib.xdtts_griffinlim_timbre_linear_batch(None, sp, nf, 0, ta, op) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_timbre_linear_batch(None, sp, nf, 3, None, op) == pkg.XDTTS_ERR_BAD_ARG


def test_noise_bits_equal_the_restatement(pkg):
    """xdtts_timbre_noise_bits == the numpy n, bit for bit, on the grid."""
    for seed in (0, 1, 0xFFFFFFFF):
        for frame in (0, 1, 799, (1 << 20) - 1):
            for b in (0, 1, 511, 512):
                n = pkg.timbre_noise_bits(seed, frame, b)
                assert n == int(tr.noise_bits(seed, frame, b)[0]), (seed, frame, b)
                assert 0 <= n < (1 << 23)
    # ... and a whole frame at once against the vectorised form the reference uses
    ref = tr.noise_bits(7, np.arange(3)[:, None], np.arange(tr.NB)[None, :])
    got = np.array([[pkg.timbre_noise_bits(7, j, k) for k in range(tr.NB)] for j in range(3)], dtype=np.uint32)
    assert np.array_equal(ref, got)


def test_noise_has_zero_mean_and_the_analytic_range():
    """N over 513 x 48 cells: |mean| <= 0.02; min and max inside [0.5 ln 2^-24 + gamma / 2, 0.5 ln(24 ln 2) + gamma / 2]."""
    N = tr.noise(1, 48)
    assert N.shape == (48, tr.NB)
    print("timbre noise over %d cells: mean %+.4f, std %.4f, min %.3f, max %.3f (range %.3f .. %.3f)" %
          (N.size, N.mean(), N.std(), N.min(), N.max(), tr.N_MIN, tr.N_MAX))
    assert abs(float(N.mean())) <= 0.02
    assert tr.N_MIN - 1e-6 <= float(N.min()) and float(N.max()) <= tr.N_MAX + 1e-6  # (1e-6: the fp32 constant against gamma / 2)
    N32 = tr.noise(1, 48, np.float32)
    assert np.abs(N32.astype(np.float64) - N).max() <= 2e-6
    # it depends on (seed, frame, bin) alone: a longer request begins with the same frames, another seed gives other values
    assert np.array_equal(tr.noise(1, 5), N[:5])
    assert not np.array_equal(tr.noise(2, 5), N[:5])


def test_properties_of_the_reference():
    """Period 157 unchanged for vtl 0.8 / 1.25 / 1.5; cepstral-peak ratio <= 0.25 at breath 1 and in [0.4, 0.65] at breath 0.5;
    the bump's power centroid within 0.5 bin of centre / vtl for the six factors and both centres."""
    lines = []
    fig = tr.check_properties(lambda S, vtl, breath: tr.timbre(S, vtl=vtl, breath=breath), say=lines.append)
    print("timbre reference: " + "; ".join(lines))
    assert len(fig) == 3 + 3 + 2 + 12


def test_identity_through_the_arithmetic_path():
    """vtl == 1, breath == 0 through the arithmetic reproduces max(S, log_floor) to 1e-6 relative; the identity itself returns S."""
    S = tr.random_magnitude(9, seed=3)
    out = tr.timbre(S, arithmetic=True)
    want = np.maximum(S.astype(np.float64), float(np.float32(1e-5)))
    err = float(np.max(np.abs(out - want) / want))
    print("timbre identity through the arithmetic: %.3e" % err)
    assert err <= 1e-6
    assert np.array_equal(tr.timbre(S), S.astype(np.float64))
    assert np.array_equal(tr.timbre(S, dtype=np.float32), S)


@pytest.mark.parametrize("vtl,breath", tr.CASES)
def test_fp32_yardstick(vtl, breath):
    """The fp32 restatement against the fp64 one under the prosody test's metric: what single precision costs (the device test
    allows four times this and 2e-5).  A-priori: the error of exp's argument is that of L (|L| <= 11.5, half an ulp each) carried
    through two 1024-point transforms of ten butterfly levels -- about 11.5 x 2^-24 x sqrt(20) = 3e-6 -- and the output's
    relative error is that argument error; 2e-5 leaves a factor of six."""
    S = tr.random_magnitude(37)
    ref = tr.timbre(S, vtl=vtl, breath=breath)
    d32 = tr.rel_err(tr.timbre(S, vtl=vtl, breath=breath, dtype=np.float32), ref)
    print("timbre fp32 against fp64, vtl %g breath %g: %.3e" % (vtl, breath, d32))
    assert np.all(np.isfinite(ref)) and np.all(ref > 0)
    assert d32 <= 2e-5


def test_vtl_leaves_the_fine_structure_and_breath_the_envelope():
    """The split of the output: under vtl alone R' == R; under breath alone E' == E (the reference's own cepstral split, fp64)."""
    S = tr.random_magnitude(5, seed=2)
    m = np.arange(tr.N_FFT)
    ext = np.minimum(m, tr.N_FFT - m)

    def split(X):
        L = np.log(np.maximum(X.T, float(np.float32(1e-5))))
        c = np.fft.fft(L[:, ext], axis=1).real / tr.N_FFT
        c[:, (m > 30) & (m < tr.N_FFT - 30)] = 0
        E = np.fft.fft(c, axis=1).real[:, : tr.NB]
        return E, L - E

    E0, R0 = split(S.astype(np.float64))
    out = tr.timbre(S, vtl=1.0, breath=0.6)
    L1 = np.log(out.T)
    want = E0 + 0.4 * R0 + 0.6 * tr.noise(1, 5)
    assert np.abs(L1 - want).max() <= 1e-5  # (fp32 parameters: 0.6f is not 0.6)


# ---- the stand-alone driver ------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_timbre_plan_driver_under_sanitizers(tmp_path):
    """tests/timbre_plan_test.cpp with plain g++ and -fsanitize=address,undefined: the argument rules (each bound, NaN, inf), the
    identity test, n / v / N at the grid's corners."""
    exe = str(tmp_path / "timbre_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "timbre_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "timbre_plan.h"), encoding="utf-8").read()
    assert re.findall(r"#\s*include\s*\"([^\"]+)\"", src) == ["rng.h"]  # of the library's headers, the other plain one
    assert not re.search(r"#\s*include\s*<hip/", src)
