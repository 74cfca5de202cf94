"""The dynamic range compressor without a device (include/xdtts.h; csrc/compressor_plan.h): the bindings and argument rules, the
host integers, lvl and the integer envelope against the fp64 / integer restatement (tests/compressor_ref.py, which uses the
serial recurrences), xdtts_compressor_reference against the restatement under an a-priori bound, the properties of its output,
and the sanitizer-built stand-alone driver of the plan header."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import compressor_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ["xdtts_compressor_default", "xdtts_compressor_preset", "xdtts_griffinlim_set_compressor", "xdtts_griffinlim_get_compressor",
       "xdtts_griffinlim_last_compressor", "xdtts_griffinlim_compress", "xdtts_griffinlim_compress_batch", "xdtts_compressor_plan",
       "xdtts_compressor_level", "xdtts_compressor_envelope", "xdtts_compressor_reference"]


def _comp(pkg, **kw):
    return pkg.Compressor(**dict(cr.DRC, **kw))


def test_symbols_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "xdtts.h")).read()
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in pkg.SYMBOLS, name
    for attr in ("set_compressor", "get_compressor", "last_compressor", "compress", "compress_batch"):
        assert callable(getattr(pkg.GriffinLim, attr))
    for attr in ("compressor_plan", "compressor_level", "compressor_envelope", "compressor_reference", "compressor_preset"):
        assert callable(getattr(pkg, attr))
    assert C.sizeof(pkg.Compressor) == 24 and [f[0] for f in pkg.Compressor._fields_] == list(cr.FIELDS)
    assert C.sizeof(pkg.CompressorStats) == 24 and pkg.CompressorStats.compressed.offset == 16
    m = re.search(r"typedef struct \{([^}]*)\}\s*xdtts_compressor\s*;", header)
    assert m and re.findall(r"float\s+(\w+);", m.group(1)) == list(cr.FIELDS)
    assert re.search(r"}\s*xdtts_compressor_stats\s*;", header)
    assert pkg.Compressor().astuple() == tuple(cr.DEFAULT[k] for k in cr.FIELDS)
    assert pkg.compressor_preset(1).astuple() == tuple(cr.DRC[k] for k in cr.FIELDS)
    assert pkg.compressor_preset(0).astuple() == pkg.Compressor().astuple()
    assert pkg.lib.xdtts_compressor_preset(2, C.byref(pkg.Compressor())) == pkg.XDTTS_ERR_BAD_ARG


def test_argument_errors_are_status_codes(pkg):
    """before a device is touched: this machine has none.  Every field at both ends of its range is accepted; just outside, NaN and
    the infinities are BAD_ARG with the field's name in the message."""
    x = np.zeros(10, dtype=np.float32)
    out = np.zeros(10, dtype=np.float32)
    V = np.zeros(10, dtype=np.int32)
    st = pkg.CompressorStats()

    def ref(c, n=10, rate=22050, a=x, o=out, s=C.byref(st)):
        return pkg.lib.xdtts_compressor_reference(None if a is None else a.ctypes.data, n, rate, None if c is None else C.byref(c),
                                                  None if o is None else o.ctypes.data, s)

    assert ref(_comp(pkg)) == 0 and ref(_comp(pkg), s=None) == 0   # stats may be NULL
    for name in cr.FIELDS:
        lo, hi = cr.RANGES[name]
        for v in (lo, hi):
            assert ref(_comp(pkg, **{name: v})) == 0, (name, v)
        for v in (np.nextafter(np.float32(lo), np.float32(-np.inf)), np.nextafter(np.float32(hi), np.float32(np.inf)), float("nan"), float("inf"),
                  float("-inf")):
            bad = _comp(pkg, **{name: float(v)})
            for f in (lambda: ref(bad), lambda: pkg.lib.xdtts_compressor_plan(22050, C.byref(bad), None, None, None, None, None),
                      lambda: pkg.lib.xdtts_compressor_envelope(x.ctypes.data, 10, 22050, C.byref(bad), V.ctypes.data),
                      lambda: pkg.lib.xdtts_griffinlim_set_compressor(None, C.byref(bad)),   # the fields first, then the handle
                      lambda: pkg.lib.xdtts_griffinlim_compress(None, x.ctypes.data, 10, 22050, C.byref(bad), out.ctypes.data, C.byref(st))):
                assert f() == pkg.XDTTS_ERR_BAD_ARG, (name, v)
                assert name in pkg.lib.xdtts_last_error().decode(), (name, v)
    ok = _comp(pkg)
    for kw in (dict(n=0), dict(n=1 << 28), dict(rate=7999), dict(rate=96001), dict(a=None), dict(o=None), dict(c=None)):
        a = dict(c=ok)
        a.update(kw)
        assert ref(**a) == pkg.XDTTS_ERR_BAD_ARG, kw
    assert pkg.lib.xdtts_compressor_plan(22050, C.byref(ok), None, None, None, None, None) == 0   # any out pointer may be NULL
    assert pkg.lib.xdtts_compressor_plan(7999, C.byref(ok), None, None, None, None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_compressor_plan(22050, None, None, None, None, None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_compressor_level(None, 5, V.ctypes.data) == pkg.XDTTS_ERR_BAD_ARG
    # a NULL handle is rejected before a device is touched, with good arguments too
    assert pkg.lib.xdtts_griffinlim_set_compressor(None, C.byref(ok)) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_set_compressor(None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_get_compressor(None, C.byref(ok), None) == pkg.XDTTS_ERR_BAD_ARG
    n = C.c_size_t()
    assert pkg.lib.xdtts_griffinlim_last_compressor(None, None, 0, C.byref(n)) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_compress(None, x.ctypes.data, 10, 22050, C.byref(ok), out.ctypes.data, C.byref(st)) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_compress(None, x.ctypes.data, 10, 22050, C.byref(pkg.Compressor()), out.ctypes.data, C.byref(st)) == pkg.XDTTS_ERR_BAD_ARG


@pytest.mark.parametrize("Q", (8000, 11025, 22050, 44100, 48000, 96000))
def test_plan_equals_the_restatement(pkg, Q):
    """alpha, rho, T, W exactly; the ends of the slopes' range: 0.1 ms at 8 kHz (the steepest slope any setting gives, below the
    clamp at 2^18) and 2000 ms at 96 kHz (the clamp at 1)."""
    cases = [cr.DRC, dict(cr.DRC, attack_ms=0.1, release_ms=2000.0), dict(cr.DRC, attack_ms=100.0, release_ms=1.0),
             dict(threshold_db=-60.0, ratio=20.0, knee_db=24.0, attack_ms=0.37, release_ms=777.7, makeup_db=24.0),
             dict(threshold_db=-0.001, ratio=1.0, knee_db=0.0, attack_ms=33.3, release_ms=1999.9, makeup_db=0.5)]
    for kw in cases:
        c = cr.settings(**kw)
        got = pkg.compressor_plan(Q, pkg.Compressor(**kw))
        assert got == cr.plan(Q, c), (Q, kw)
        assert 1 <= got["alpha"] <= 1 << 18 and 1 <= got["rho"] <= 1 << 18 and got["T"] <= 0 <= got["W"] and got["tile"] == 4096
    ends = pkg.Compressor(**dict(cr.DRC, attack_ms=0.1, release_ms=2000.0))
    assert pkg.compressor_plan(8000, ends)["alpha"] == cr.slope(float(np.float32(0.1)), 8000) == 136066
    assert pkg.compressor_plan(96000, ends)["rho"] == 1 and 65536.0 * (10.0 / (20.0 * cr.LOG10_2)) / 192000.0 < 1.0   # clamped from 0.57


def test_level_against_fp64(pkg):
    """|lvl(a) - 65536 log2 a| <= LVL_BOUND = 0.5614 units for every normal float (compressor_ref.py: how it is derived -- the
    polynomial's stated error, the fmaf roundings, the rounding to an integer; never tuned to the output).  The two premises
    about the polynomial are recomputed here in fp64 from the coefficients the header names: its error in exact arithmetic and
    the size of Horner's partial values.  Worst observed / bound: 0.90 (the rounding to an integer alone is 0.89 of it)."""
    f = np.linspace(0.0, 1.0, 400001)
    acc = np.full_like(f, cr.LOG2_Q[-1])
    biggest = np.abs(acc).max()
    for ck in cr.LOG2_Q[-2::-1]:
        acc = acc * f + ck
        biggest = max(biggest, np.abs(acc).max())
    assert np.abs(acc * f - np.log2(1.0 + f)).max() <= cr.LOG2_POLY_ERR and biggest <= 1.45
    rng = np.random.Generator(np.random.PCG64(5))
    mant = np.concatenate([np.linspace(1.0, 2.0, 300001)[:-1], 1.0 + rng.random(200000)])
    x = np.concatenate([mant, mant * 2.0 ** -20, -mant * 2.0 ** 7, mant[:1000] * 2.0 ** -126, mant[:1000] * 2.0 ** 127]).astype(np.float32)
    l = pkg.compressor_level(x).astype(np.float64)
    err = np.abs(l - 65536.0 * np.log2(np.abs(x.astype(np.float64))))
    print("compressor lvl against 65536 log2: worst |error| = %.4f units, %.3f of the bound %.4f" % (err.max(), err.max() / cr.LVL_BOUND, cr.LVL_BOUND))
    assert err.max() <= cr.LVL_BOUND < 1.0
    # the exact points, and the floor
    ex = np.array([1.0, -1.0, 0.5, 2.0, 2.0 ** -126, 0.0, -0.0, 1e-40, 2.0 ** -127], dtype=np.float32)
    assert list(pkg.compressor_level(ex)) == [0, 0, -65536, 65536, -126 * 65536] + [cr.L_FLOOR] * 4
    assert np.abs(pkg.compressor_level(x) - cr.level(x)).max() <= 1   # what gain_bound builds on


@functools.lru_cache(maxsize=None)
def _case(kind, Q):
    """(input, the library's level): computed once, shared, never written to"""
    import importlib

    pkg = importlib.import_module("xd-tts_amd")
    x = cr.signal(kind, Q, 2 * cr.TILE + 301)
    x.setflags(write=False)
    l = pkg.compressor_level(x)
    l.setflags(write=False)
    return x, l


SETTINGS = (cr.DRC, dict(cr.DRC, ratio=20.0, knee_db=0.0, attack_ms=0.1, release_ms=1.0), dict(cr.DRC, ratio=1.5, knee_db=24.0, attack_ms=100.0, release_ms=2000.0))


@pytest.mark.parametrize("Q", cr.RATES)
@pytest.mark.parametrize("kind", cr.KINDS)
def test_envelope_equals_the_restatement(pkg, kind, Q):
    """xdtts_compressor_envelope == the serial recurrences over the library's own l, every integer."""
    x, l = _case(kind, Q)
    for kw in SETTINGS:
        p = cr.plan(Q, cr.settings(**kw))
        V = pkg.compressor_envelope(x, Q, pkg.Compressor(**kw))
        assert np.array_equal(V.astype(np.int64), cr.envelope(l, p["alpha"], p["rho"])), (kind, Q, kw)
        assert np.all(V >= l) and V.max() == l.max() and V.min() >= cr.L_FLOOR


@pytest.mark.parametrize("Q", cr.RATES)
def test_reference_against_fp64(pkg, Q):
    """|out - out64| <= |out64| B with B = compressor_ref.gain_bound (how it is derived: two units of level through a gain
    computer of slope <= |s|, its fp32 roundings, the 2^x polynomial, the products), out64 the restatement with its OWN fp64
    level.  compressed and max_over equal the restatement's when it is given the library's l.  Worst ratio to the bound over
    the 60 cases: 0.47, recorded in profiles/compressor.txt."""
    worst = 0.0
    for kind in cr.KINDS:
        x, l = _case(kind, Q)
        for kw in SETTINGS + (dict(cr.DRC, makeup_db=6.0),):
            c = cr.settings(**kw)
            out, st = pkg.compressor_reference(x, Q, pkg.Compressor(**kw))
            ref = cr.compress(x, Q, c)
            B = cr.gain_bound(Q, c)
            err, lim = np.abs(out.astype(np.float64) - ref["out"]), np.abs(ref["out"]) * B
            assert np.all(err <= lim), (kind, Q, kw, float((err / np.maximum(lim, 1e-300)).max()))
            worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
            same_l = cr.compress(x, Q, c, l=l)
            assert (st.engaged, st.compressed, st.max_over) == (1, same_l["compressed"], same_l["max_over"]), (kind, Q, kw)
            assert st.max_over == -same_l["plan"]["T"] and st.peak == np.abs(x).max()
            # the gain never exceeds mk
            assert np.all(np.abs(out) <= np.abs(x * np.float32(ref["mk"]))), (kind, Q, kw)
    print("compressor reference against fp64, rate %d: worst |out - out64| / bound = %.4f" % (Q, worst))


def _gain_db(out, x, mk=1.0):
    return 20.0 * np.log10(np.abs(out.astype(np.float64)) / (np.abs(x.astype(np.float64)) * mk))


@pytest.mark.parametrize("Q", cr.RATES)
@pytest.mark.parametrize("mk_db", (0.0, 6.0))
def test_two_level_signal(pkg, Q, mk_db):
    """A loud half at the peak and a quiet half 40 dB under it (threshold -24, knee 6: below the knee's foot at -27 by more than
    the knee).  The release tent falls from the boundary to the knee's foot in 2.7 release_ms, the attack tent in 2.7 attack_ms:
    further than that from the boundary the loud half is reduced by (1 - 1 / ratio) 24 dB = 16 dB within 0.05 dB plus the bound,
    and the quiet half is fl(x mk) bit for bit."""
    kw = dict(cr.DRC, makeup_db=mk_db, release_ms=20.0)
    c = cr.settings(**kw)
    B_db = 20.0 * np.log10(1.0 + cr.gain_bound(Q, c))
    N = int(0.08 * Q)
    reach_r, reach_a = int(2.7 * 20.0 * Q / 1000.0) + 2, int(2.7 * 5.0 * Q / 1000.0) + 2
    mk = np.float32(10.0 ** (mk_db / 20.0))
    for loud_first in (True, False):
        x = cr.two_level(N, loud_first=loud_first)
        out, st = pkg.compressor_reference(x, Q, pkg.Compressor(**kw))
        loud = slice(0, N) if loud_first else slice(N, 2 * N)
        quiet = slice(N + reach_r, 2 * N) if loud_first else slice(0, N - reach_a)
        g = _gain_db(out[loud], x[loud], float(mk))
        assert np.abs(g + (1.0 - 1.0 / 3.0) * 24.0).max() <= 0.05 + B_db, (Q, loud_first)
        assert np.array_equal((x * mk)[quiet].view(np.uint32), out[quiet].view(np.uint32)), (Q, loud_first)
        assert quiet.stop - quiet.start > N // 4
        assert np.all(np.abs(out) <= np.abs(x * mk))   # the gain never exceeds mk


@pytest.mark.parametrize("Q", cr.RATES)
def test_attack_and_release_slopes(pkg, Q):
    """In front of a loud onset the gain in dB falls by 10 dB (1 - 1 / ratio) per attack_ms, behind the loud stretch it recovers
    by as much per release_ms: measured over the stretch where the tent is above the knee (21 dB of envelope), to within one
    slope unit (alpha and rho are integers: 1 / alpha, 1 / rho of the figure) plus the bound at the two ends of the stretch."""
    ratio = 3.0
    for att, rel in ((5.0, 20.0), (1.0, 10.0)):
        kw = dict(cr.DRC, attack_ms=att, release_ms=rel)
        c = cr.settings(**kw)
        p = cr.plan(Q, c)
        B_db = 20.0 * np.log10(1.0 + cr.gain_bound(Q, c))
        N = int(0.1 * Q)
        x = np.concatenate([cr.two_level(N, quiet_db=-60.0, loud_first=False), cr.two_level(N, quiet_db=-60.0)[N:]])   # quiet, loud, quiet
        out, _ = pkg.compressor_reference(x, Q, pkg.Compressor(**kw))
        g = _gain_db(out, x)
        want = 10.0 * (1.0 - 1.0 / ratio)
        for slope, ms, edge, sign in ((p["alpha"], att, N - 1, -1), (p["rho"], rel, 2 * N, 1)):
            d = int((-p["T"] - p["W"] / 2.0) / slope) - 1          # samples the tent stays above the knee
            assert d >= 4
            a, b = edge, edge + sign * d                           # the first quiet sample next to the loud stretch, and d further
            per_ms = abs(g[b] - g[a] - 0.0) / d * (ms * Q / 1000.0)
            # the first quiet sample is one slope step under the loud level already: both ends lie on the tent
            assert abs(per_ms - want) <= want / slope + 2.0 * B_db * (ms * Q / 1000.0) / d, (Q, att, rel, sign, per_ms)


def test_identity_and_silence(pkg):
    x = cr.signal("impulses", 22050, 5000)
    out, st = pkg.compressor_reference(x, 22050, pkg.Compressor())
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32)) and st.astuple() == (0.0, 0, 0, 0)
    out, st = pkg.compressor_reference(x, 22050, pkg.Compressor(threshold_db=-30.0, knee_db=12.0))   # ratio 1, makeup 0: still the identity
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32)) and st.engaged == 0
    z = np.zeros(5000, dtype=np.float32)
    z[3] = -0.0
    out, st = pkg.compressor_reference(z, 22050, pkg.compressor_preset(1))
    assert np.array_equal(out.view(np.uint32), z.view(np.uint32)) and st.astuple() == (0.0, 0, 0, 0)
    assert cr.compress(z, 22050, cr.settings(**cr.DRC))["engaged"] == 0


# ---- the stand-alone driver ------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_compressor_plan_driver_under_sanitizers(tmp_path):
    """tests/compressor_plan_test.cpp with plain g++ and -fsanitize=address,undefined: the rules, the host integers, and the two
    passes over a tile as the workgroups of k_comp_tiles and k_compress perform them, into buffers of the exact size, against the
    sample-by-sample reference at the shapes the GPU tests use."""
    exe = str(tmp_path / "compressor_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "compressor_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "compressor_plan.h"), encoding="utf-8").read()
    assert re.findall(r"#\s*include\s*\"([^\"]+)\"", src) == []   # none of the library's headers
    assert not re.search(r"#\s*include\s*<hip/", src)
    for libm in ("log2f", "exp2f", "powf", "logf(", "expf("):
        assert libm not in src, libm
