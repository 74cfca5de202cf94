"""The silence stage without a device (include/xdtts.h; csrc/silence_plan.h): the exports and bindings, the struct sizes read from
the header, every argument rule by field name, the host integers at seven rates, xdtts_silence_keep and xdtts_silence_reference
against the numpy restatement (tests/silence_ref.py) bit for bit on the crafted signals, the properties of the output, and the
sanitizer-built stand-alone driver of the plan header."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import silence_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ["xdtts_silence_default", "xdtts_griffinlim_set_silence", "xdtts_griffinlim_get_silence", "xdtts_griffinlim_last_silence",
       "xdtts_griffinlim_trim", "xdtts_griffinlim_trim_batch", "xdtts_silence_plan", "xdtts_silence_keep", "xdtts_silence_reference"]
C_SIZES = {"float": 4, "uint32_t": 4, "int32_t": 4}


def _sil(pkg, s=None, **kw):
    return pkg.Silence(**dict(s or sr.DEFAULT, **kw))


def _plan(pkg, rate, s):
    got = pkg.silence_plan(rate, _sil(pkg, s))
    return got, sr.plan(rate, s, got["tfac"])


@functools.lru_cache(maxsize=None)
def _cases():
    return sr.cases()


CASE_IDS = [c[0] for c in sr.cases()]


def _struct_fields(header, name):
    """[(type, field)] of `typedef struct { ... } name;` in the header, comments removed"""
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s\s*;" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, name
    out = []
    for typ, names in re.findall(r"(\w+)\s+([\w\s,]+);", m.group(1)):
        out += [(typ, f.strip()) for f in names.split(",")]
    return out


def test_symbols_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "xdtts.h")).read()
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in pkg.SYMBOLS, name
    for attr in ("set_silence", "get_silence", "last_silence", "trim", "trim_batch"):
        assert callable(getattr(pkg.GriffinLim, attr))
    for attr in ("silence_plan", "silence_keep", "silence_reference"):
        assert callable(getattr(pkg, attr))
    # the sizes, from the header
    fs = _struct_fields(header, "xdtts_silence")
    assert [f for _t, f in fs] == list(sr.FIELDS) and sum(C_SIZES[t] for t, _f in fs) == 24 == C.sizeof(pkg.Silence)
    assert [f[0] for f in pkg.Silence._fields_] == list(sr.FIELDS)
    fs = _struct_fields(header, "xdtts_silence_stats")
    assert [f for _t, f in fs] == list(sr.STATS) and sum(C_SIZES[t] for t, _f in fs) == 32 == C.sizeof(pkg.SilenceStats)
    assert [f[0] for f in pkg.SilenceStats._fields_] == list(sr.STATS)
    assert pkg.Silence().astuple() == tuple(sr.DEFAULT[k] for k in sr.FIELDS)
    hpp = open(os.path.join(ROOT, "include", "xdtts_host.hpp")).read()
    for name in ("set_silence", "silence_setting", "last_silence", "trim"):
        assert re.search(r"\b%s\s*\(" % name, hpp), name


def test_argument_errors_are_status_codes(pkg):
    """before a device is touched: this machine has none.  Every field at both ends of its range is accepted; just outside, NaN and
    the infinities are BAD_ARG with the field's name in the message, on every entry that takes the struct."""
    x = np.full(10, 0.5, dtype=np.float32)
    out = np.zeros(10, dtype=np.float32)
    keep = np.zeros(4, dtype=np.uint8)
    st = pkg.SilenceStats()

    def ref(s, n=10, rate=22050, a=x, o=out, t=C.byref(st)):
        return pkg.lib.xdtts_silence_reference(None if a is None else a.ctypes.data, n, rate, None if s is None else C.byref(s),
                                               None if o is None else o.ctypes.data, t)

    assert ref(_sil(pkg)) == 0 and ref(_sil(pkg), t=None) == 0   # stats may be NULL
    for name in sr.FIELDS:
        lo, hi = sr.RANGES[name]
        for v in (lo, hi):
            assert ref(_sil(pkg, **{name: v})) == 0, (name, v)
        for v in (np.nextafter(np.float32(lo), np.float32(-np.inf)), np.nextafter(np.float32(hi), np.float32(np.inf)), float("nan"), float("inf"),
                  float("-inf")):
            bad = _sil(pkg, **{name: float(v)})
            for f in (lambda: ref(bad), lambda: pkg.lib.xdtts_silence_plan(22050, C.byref(bad), *([None] * 7)),
                      lambda: pkg.lib.xdtts_silence_keep(x.ctypes.data, 10, 22050, C.byref(bad), keep.ctypes.data),
                      lambda: pkg.lib.xdtts_griffinlim_set_silence(None, C.byref(bad)),   # the fields first, then the handle
                      lambda: pkg.lib.xdtts_griffinlim_trim(None, x.ctypes.data, 10, 22050, C.byref(bad), out.ctypes.data, C.byref(st))):
                assert f() == pkg.XDTTS_ERR_BAD_ARG, (name, v)
                assert name in pkg.lib.xdtts_last_error().decode(), (name, v)
    assert ref(_sil(pkg, max_pause_ms=0.0)) == 0 and ref(_sil(pkg, max_pause_ms=10.0)) == pkg.XDTTS_ERR_BAD_ARG
    assert "max_pause_ms" in pkg.lib.xdtts_last_error().decode()
    ok = _sil(pkg)
    for kw, word in ((dict(n=0), "n"), (dict(n=1 << 28), "n"), (dict(rate=7999), "rate"), (dict(rate=96001), "rate"), (dict(a=None), "null"),
                     (dict(o=None), "null"), (dict(o=x), "out"), (dict(s=None), "null")):
        a = dict(s=ok)
        a.update(kw)
        assert ref(**a) == pkg.XDTTS_ERR_BAD_ARG, kw
        assert word in pkg.lib.xdtts_last_error().decode(), kw
    assert pkg.lib.xdtts_silence_plan(22050, C.byref(ok), *([None] * 7)) == 0   # any out pointer may be NULL
    assert pkg.lib.xdtts_silence_plan(7999, C.byref(ok), *([None] * 7)) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_silence_plan(22050, None, *([None] * 7)) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_silence_keep(x.ctypes.data, 10, 22050, C.byref(ok), None) == pkg.XDTTS_ERR_BAD_ARG
    # a NULL handle is rejected before a device is touched, with good arguments too
    n = C.c_size_t()
    assert pkg.lib.xdtts_griffinlim_set_silence(None, C.byref(ok)) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_set_silence(None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_get_silence(None, C.byref(ok), None) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_last_silence(None, None, 0, C.byref(n)) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_trim(None, x.ctypes.data, 10, 22050, C.byref(ok), out.ctypes.data, C.byref(st)) == pkg.XDTTS_ERR_BAD_ARG
    ptrs = (C.c_void_p * 1)(x.ctypes.data)
    outs = (C.c_void_p * 1)(out.ctypes.data)
    for ns, rate in (((C.c_size_t * 1)(0), 22050), ((C.c_size_t * 1)(10), 5000)):
        assert pkg.lib.xdtts_griffinlim_trim_batch(None, ptrs, ns, 1, rate, C.byref(ok), outs, C.byref(st)) == pkg.XDTTS_ERR_BAD_ARG
        assert "utterance 0" in pkg.lib.xdtts_last_error().decode()


@pytest.mark.parametrize("Q", sr.RATES)
def test_plan_equals_the_restatement(pkg, Q):
    """W, the settings in windows and the fade, exactly, at the seven rates; tfac is the float of 10^(dB / 20)."""
    W = {8000: 40, 11025: 55, 16000: 80, 22050: 110, 44100: 220, 48000: 240, 96000: 480}[Q]
    sets = [sr.settings(), sr.settings(min_sound_ms=12.5, lead_ms=2.4, trail_ms=7.5, max_pause_ms=105.0, fade_ms=2.5),
            sr.settings(threshold_db=-96.0, min_sound_ms=500.0, lead_ms=10000.0, trail_ms=10000.0, max_pause_ms=60000.0, fade_ms=0.0),
            sr.settings(threshold_db=-6.0, min_sound_ms=0.0, lead_ms=0.0, trail_ms=0.0, max_pause_ms=20.0, fade_ms=0.3),
            sr.settings(min_sound_ms=17.3, lead_ms=1234.5, trail_ms=77.7, max_pause_ms=333.3, fade_ms=1.1)]
    for s in sets:
        got, want = _plan(pkg, Q, s)
        assert got == want and got["W"] == W, (Q, s, got, want)
        assert abs(float(got["tfac"]) / 10.0 ** (float(np.float32(s["threshold_db"])) / 20.0) - 1.0) <= 2.0 ** -24
        assert 0 <= got["fade"] <= W // 2
    got, _ = _plan(pkg, Q, sets[0])
    assert (got["min_w"], got["lead_w"], got["trail_w"], got["pause_w"]) == (4, 10, 20, 0)
    assert _plan(pkg, Q, sets[1])[0]["pause_w"] == 21   # odd


def _stats(st):
    return st.astuple()


@pytest.mark.parametrize("case", range(len(CASE_IDS)), ids=CASE_IDS)
def test_keep_and_reference_equal_the_restatement(pkg, case):
    """xdtts_silence_keep and xdtts_silence_reference against the serial restatement: every decision, every sample's bits and
    every field of the stats; and the properties of the output."""
    name, Q, s, x = _cases()[case]
    got, p = _plan(pkg, Q, s)
    assert got == p
    keep_ref, sound, P = sr.decisions(x, p)
    keep = pkg.silence_keep(x, Q, _sil(pkg, s))
    assert keep.tolist() == [int(k) for k in keep_ref], name
    out, st = pkg.silence_reference(x, Q, _sil(pkg, s))
    want, wst = sr.reference(x, p)
    assert _stats(st) == wst, (name, _stats(st), wst)
    assert out.size == st.n_out and np.array_equal(out.view(np.uint32), want.view(np.uint32)), name
    assert st.n_out + st.lead_cut + st.trail_cut + st.pause_cut == st.n_in == x.size
    # every sound window survives unmodified except inside fades
    W, fade, nw, at = p["W"], p["fade"], len(keep_ref), 0
    for w in range(nw):
        n_w = min(x.size, (w + 1) * W) - w * W
        if not keep_ref[w]:
            assert not sound[w]
            continue
        if sound[w]:
            lo = fade if w > 0 and not keep_ref[w - 1] else 0
            hi = n_w - (fade if w < nw - 1 and not keep_ref[w + 1] else 0)
            assert np.array_equal(out[at + lo:at + hi].view(np.uint32), x[w * W + lo:w * W + hi].view(np.uint32)), (name, w)
        at += n_w
    assert np.max(np.abs(out), initial=0.0) <= st.peak


def test_what_the_crafted_signals_exercise(pkg):
    """the cases do what their names say: the click of min_w - 1 windows is dropped and the one of min_w kept; a pause of pause_w
    windows is left alone and one of pause_w + 1 shortened to pause_w; lead and trail beyond what is there keep everything."""
    by = {c[0]: c for c in _cases()}
    _n, Q, s, x = by["clicks"]
    out, st = pkg.silence_reference(x, Q, _sil(pkg, s))
    W = 110
    assert st.any_sound == 1 and st.lead_cut == (30 + 3 + 30 - 10) * W and st.trail_cut == 21 * W + 7 and st.pause_cut == 0 and st.n_cuts == 2
    for name in ("pauses even", "pauses odd", "pauses even noise", "pauses odd noise"):
        _n, Q, s, x = by[name]
        pz = sr.win(s["max_pause_ms"])
        out, st = pkg.silence_reference(x, Q, _sil(pkg, s))
        assert st.pause_cut == (1 + 2 * pz) * W and st.lead_cut == 3 * W and st.trail_cut == 5 * W + 50 and st.n_cuts == 2 + 2 * 2, name
    _n, Q, s, x = by["lead and trail past the ends"]
    out, st = pkg.silence_reference(x, Q, _sil(pkg, s))
    assert st.n_out == x.size and st.n_cuts == 0 and np.array_equal(out.view(np.uint32), x.view(np.uint32))
    _n, Q, s, x = by["zeros"]
    out, st = pkg.silence_reference(x, Q, _sil(pkg, s))
    assert st.any_sound == 0 and st.peak == 0.0 and st.n_out == 30 * W and st.trail_cut == 5000 - 30 * W and not out.any()
    _n, Q, s, x = by["short last window"]
    out, st = pkg.silence_reference(x, Q, _sil(pkg, s))
    assert st.n_out == 10 + 20 * 0 and st.lead_cut == 40 * W and st.n_cuts == 1 and np.all(np.abs(out) < np.abs(x[-10:]))
    _n, Q, s, x = by["1200 windows"]
    assert x.size == 132000 and -(-x.size // W) == 1200


def test_identity_with_everything_kept(pkg):
    """max_pause_ms = 0 with lead and trail at their maxima: the output is the input, whatever it holds"""
    s = sr.settings(lead_ms=10000.0, trail_ms=10000.0)
    for _n, Q, _s, x in _cases():
        if not x.any():
            continue
        out, st = pkg.silence_reference(x, Q, _sil(pkg, s))
        assert st.n_out == x.size and st.n_cuts == 0 and np.array_equal(out.view(np.uint32), x.view(np.uint32))


# ---- the stand-alone driver ------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_silence_plan_driver_under_sanitizers(tmp_path):
    """tests/silence_plan_test.cpp with plain g++ and -fsanitize=address,undefined: the rules, the host integers, and the three
    launches as the workgroups perform them, into buffers of the exact size, against the serial definition."""
    exe = str(tmp_path / "silence_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "silence_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "silence_plan.h"), encoding="utf-8").read()
    assert sorted(re.findall(r"#\s*include\s*\"([^\"]+)\"", src)) == ["resample_plan.h", "stream_plan.h"]   # both plain host C++
    assert not re.search(r"#\s*include\s*<hip/", src)
