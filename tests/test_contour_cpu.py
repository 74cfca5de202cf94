"""CPU-only checks of the prosody contour entries (rate, pitch and gain that vary inside an utterance): declared, bound, exported
and mirrored; the host table (xd-tts_amd/csrc/prosody_contour.h) against its numpy restatement bit for bit; every argument rule
as a status code before any device is touched; the stand-alone C++ driver of the header; and the numpy restatement
(tests/contour_ref.py), which the GPU tests take as their reference, doing what the definition promises."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contour_ref as cr
import prosody_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ("xdtts_prosody_contour_default", "xdtts_prosody_contour_frames", "xdtts_prosody_contour_table", "xdtts_griffinlim_contour_linear",
       "xdtts_griffinlim_contour_linear_batch", "xdtts_griffinlim_infer_contour", "xdtts_griffinlim_infer_batch_contour",
       "xdtts_synthesize_ids_contour", "xdtts_synthesize_batch_contour")
FRAMES = (2, 3, 5, 37, 800, 16384)


def random_contours(n=60, seed=7):
    """Seeded random contours: 1 .. 8 points, sorted positions (some repeated: steps; some at 0 and 1), fields over their ranges."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(1, 9))
        pos = np.sort(rng.choice(np.array([0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.5, 0.77, 1.0, rng.random(), rng.random()]), size=k))
        out.append([(float(p), float(rng.uniform(0.25, 4.0)), float(rng.choice([1.0, rng.uniform(0.5, 2.0)])), float(rng.choice([0.0, 1.0, rng.uniform(0.0, 8.0)])))
                    for p in pos])
    return out


def test_contour_symbols_are_declared_bound_exported_and_mirrored(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdtts.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.LIB_PATH)
    host = open(os.path.join(ROOT, "include", "xdtts_host.hpp")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), "include/xdtts.h does not declare %s" % name
        assert name in pkg.SYMBOLS and hasattr(raw, name), name
        assert name in host, "include/xdtts_host.hpp does not mirror %s" % name
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+pos,\s*rate,\s*pitch,\s*gain;\s*\}\s*xdtts_prosody_point;", text)
    assert re.search(r"typedef\s+struct\s*\{[^}]*\bpoints;[^}]*\bn_points;[^}]*\blifter;[^}]*\blog_floor;[^}]*\}\s*xdtts_prosody_contour;", text)
    for method in ("contour_linear", "contour_linear_batch", "infer_contour"):
        assert callable(getattr(pkg.GriffinLim, method))
    for fn in (pkg.synthesize, pkg.synthesize_batch, pkg.GriffinLim.infer_batch):
        assert "contour" in fn.__code__.co_varnames and "prosody" in fn.__code__.co_varnames
    assert callable(pkg.prosody_contour_frames) and callable(pkg.prosody_contour_table)


def test_sizes_and_defaults(pkg):
    assert C.sizeof(pkg.ProsodyPoint) == 16 and C.sizeof(pkg.Prosody) == 16
    c = pkg.ProsodyContour([(0.0, 2.0, 1.0, 1.0)])
    c.lifter, c.log_floor = 9, 9.0
    pkg.lib.xdtts_prosody_contour_default(C.byref(c))
    assert (c.n_points, c.lifter, c.log_floor, bool(c.points)) == (0, 30, float(np.float32(1e-5)), False)
    pkg.lib.xdtts_prosody_contour_default(None)  # a null pointer is ignored
    d = pkg.ProsodyContour(cr.CONTOURS["five"], lifter=40)
    assert (d.n_points, d.lifter, d.points[1].rate, d.points[4].gain) == (5, 40, 4.0, 1.5)


def test_prosody_and_contour_together_are_a_value_error(pkg):
    c, p = pkg.ProsodyContour(cr.IDENTITY), pkg.Prosody()
    with pytest.raises(ValueError):
        pkg.synthesize(None, None, np.zeros(3, np.int64), prosody=p, contour=c)
    with pytest.raises(ValueError):
        pkg.synthesize_batch(None, None, [[np.zeros(3, np.int64)]], prosody=[p], contour=[c])
    with pytest.raises(ValueError):
        pkg.GriffinLim.infer_batch(None, [np.zeros((80, 3), np.float32)], prosody=[p], contour=[c])


@pytest.mark.parametrize("F", FRAMES)
def test_table_and_frames_equal_the_numpy_table_bit_for_bit(pkg, F):
    """c, pitch and gain of xdtts_prosody_contour_table and F' of xdtts_prosody_contour_frames against contour_ref.table: the five
    named contours and sixty seeded random ones."""
    for points in list(cr.CONTOURS.values()) + random_contours():
        if cr.is_identity(points):
            continue
        con = pkg.ProsodyContour(points)
        c, pitch, gain = pkg.prosody_contour_table(con, F)
        rc, rp, rg = cr.table(points, F)
        assert c.dtype == np.uint32 and np.array_equal(c, rc), (F, points)
        assert np.array_equal(pitch, rp) and np.array_equal(gain, rg), (F, points)
        assert pkg.prosody_contour_frames(con, F) == cr.frames_of(rc[-1]) == cr.frames(points, F), (F, points)
        q = np.diff(c.astype(np.int64))
        assert q.min() >= 16384 and q.max() <= 262144


def test_table_outputs_are_optional(pkg):
    con = pkg.ProsodyContour(cr.CONTOURS["step"])
    c = np.zeros(37, np.uint32)
    assert pkg.lib.xdtts_prosody_contour_table(C.byref(con), 37, c.ctypes.data_as(C.c_void_p), None, None) == 0
    assert np.array_equal(c, cr.table(cr.CONTOURS["step"], 37)[0])
    assert pkg.lib.xdtts_prosody_contour_table(C.byref(con), 37, None, None, None) == 0


@pytest.mark.parametrize("F", FRAMES)
def test_a_rate_1_contour_maps_frame_j_to_frame_j(pkg, F):
    con = pkg.ProsodyContour([(0.0, 1.0, 1.25, 1.0), (0.5, 1.0, 0.8, 0.0)])
    c, _, _ = pkg.prosody_contour_table(con, F)
    assert np.array_equal(c, 65536 * np.arange(F, dtype=np.uint32)) and pkg.prosody_contour_frames(con, F) == F


def test_a_one_point_contour_is_within_one_frame_of_the_uniform_rate(pkg):
    """The slowness is quantised to 2^-16 frames, so F' may differ from xdtts_prosody_frames by one -- and does, at F = 3, r = 0.8."""
    seen = 0
    for F in (2, 3, 5, 37, 48, 800, 16384):
        for r in (0.25, 0.5, 0.7, 0.8, 1.0, 1.25, 1.3, 2.0, 3.3, 4.0):
            d = pkg.prosody_contour_frames(pkg.ProsodyContour([(0.0, r, 1.0, 1.0 if r != 1.0 else 0.5)]), F) - pkg.prosody_frames(F, r)
            assert abs(d) <= 1, (F, r, d)
            seen += d != 0
    assert seen >= 1
    assert pkg.prosody_contour_frames(pkg.ProsodyContour([(0.0, 0.8, 1.0, 1.0)]), 3) != pkg.prosody_frames(3, 0.8)


def test_the_identity_contour_passes_one_frame_and_many(pkg):
    ident = pkg.ProsodyContour(cr.IDENTITY)
    for F in (1, 2, 16384, 16385, 100000, 1 << 20):
        assert pkg.prosody_contour_frames(ident, F) == F
    assert pkg.prosody_contour_frames(ident, (1 << 20) + 1) == 0
    c, pitch, gain = pkg.prosody_contour_table(ident, 1)
    assert (int(c[0]), float(pitch[0]), float(gain[0])) == (0, 1.0, 1.0)
    step = pkg.ProsodyContour(cr.CONTOURS["step"])
    assert pkg.prosody_contour_frames(step, 1) == 0 and pkg.prosody_contour_frames(step, 16385) == 0
    assert pkg.prosody_contour_frames(step, 2) >= 2 and pkg.prosody_contour_frames(step, 16384) > 0
    assert pkg.lib.xdtts_prosody_contour_frames(None, 10) == 0


BAD = [([(-0.1, 1, 1, 1)], b"pos", b"point 0"), ([(0.0, 1, 1, 1), (1.5, 1, 1, 1)], b"pos", b"point 1"), ([(float("nan"), 1, 1, 1)], b"pos", b"point 0"),
       ([(0.6, 1, 1, 1), (0.5, 2, 1, 1)], b"pos", b"point 1"),
       ([(0.5, 0.2, 1, 1)], b"rate", b"point 0"), ([(0.5, 4.5, 1, 1)], b"rate", b"point 0"), ([(0.5, float("nan"), 1, 1)], b"rate", b"point 0"),
       ([(0.5, float("inf"), 1, 1)], b"rate", b"point 0"),
       ([(0.1, 1, 1, 1), (0.5, 1, 0.4, 1)], b"pitch", b"point 1"), ([(0.5, 1, 2.5, 1)], b"pitch", b"point 0"), ([(0.5, 1, float("nan"), 1)], b"pitch", b"point 0"),
       ([(0.5, 1, 1, -0.1)], b"gain", b"point 0"), ([(0.1, 1, 1, 1), (0.2, 1, 1, 1), (0.5, 1, 1, 8.5)], b"gain", b"point 2"), ([(0.5, 1, 1, float("inf"))], b"gain", b"point 0")]


def test_contour_entries_reject_bad_arguments_without_touching_a_device(pkg):
    """Every argument rule: XDTTS_ERR_BAD_ARG with the field's name (and the point's index) in the message, on the null handle,
    through each entry -- nothing is launched, so this runs without a GPU too.  The array entries name the utterance as well and
    clear their outputs."""
    lib = pkg.lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    S, out, mel = np.ones((513, 3), np.float32), np.zeros((513, 16), np.float32), np.zeros((80, 3), np.float32)
    ids, lens, uc = np.array([[64, 65, 7]], dtype=np.int64), np.array([3], np.int32), np.array([1], np.int32)
    nf, ns = C.c_size_t(7), C.c_size_t(7)
    audio, melp = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
    good = pkg.ProsodyContour(cr.CONTOURS["step"])

    def arr(c):
        a = (pkg.ProsodyContour * 2)()
        for u, x in enumerate((good, c)):
            a[u].points, a[u].n_points, a[u].lifter, a[u].log_floor = x.points, x.n_points, x.lifter, x.log_floor
        return a

    outs2, nf2 = (C.POINTER(C.c_float) * 2)(), (C.c_size_t * 2)(5, 5)
    S2, O2, n2 = (C.c_void_p * 2)(S.ctypes.data, S.ctypes.data), (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data), (C.c_size_t * 2)(3, 3)
    M2 = (C.c_void_p * 2)(mel.ctypes.data, mel.ctypes.data)
    ids2, lens2, uc2 = np.array([[64, 65, 7], [64, 65, 7]], dtype=np.int64), np.array([3, 3], np.int32), np.array([1, 1], np.int32)
    single = {
        "table": lambda c, F=3: lib.xdtts_prosody_contour_table(c, F, None, None, None),
        "linear": lambda c, F=3: lib.xdtts_griffinlim_contour_linear(None, ptr(S), F, c, ptr(out), C.byref(nf)),
        "infer": lambda c, F=3: lib.xdtts_griffinlim_infer_contour(None, ptr(mel), 80, F, c, C.byref(audio), C.byref(ns)),
        "synth": lambda c, F=3: lib.xdtts_synthesize_ids_contour(None, None, ptr(ids), 3, None, 0, None, c, C.byref(melp), C.byref(nf), C.byref(audio), C.byref(ns)),
    }
    array = {
        "linear_batch": lambda a: lib.xdtts_griffinlim_contour_linear_batch(None, S2, n2, 2, a, O2, nf2),
        "infer_batch": lambda a: lib.xdtts_griffinlim_infer_batch_contour(None, M2, 80, n2, 2, a, outs2, nf2),
        "synth_batch": lambda a: lib.xdtts_synthesize_batch_contour(None, None, ptr(ids2), ptr(lens2), 2, 3, ptr(uc2), 2, None, None, a, None, nf2, outs2, nf2),
    }

    def bad(st, *words):
        assert st == pkg.XDTTS_ERR_BAD_ARG, st
        for w in words:
            assert w in lib.xdtts_last_error(), (w, lib.xdtts_last_error())

    for name, entry in single.items():
        if name != "table":
            bad(entry(C.byref(good)), b"null")  # the null handle: the contour itself is fine
        bad(entry(None), b"null")               # the null contour
    for name, entry in array.items():
        bad(entry(arr(good)))  # the null handle
        bad(entry(None), b"null")
    for points, field, point in BAD:
        c = pkg.ProsodyContour(points)
        assert pkg.prosody_contour_frames(c, 37) == 0
        for entry in single.values():
            bad(entry(C.byref(c)), field, point)
        for entry in array.values():
            nf2[0] = nf2[1] = 5
            bad(entry(arr(c)), field, point, b"utterance 1")
            assert (nf2[0], nf2[1]) == (0, 0)
    for kw, word in ((dict(lifter=0), b"lifter"), (dict(lifter=256), b"lifter"), (dict(log_floor=0.0), b"log_floor"), (dict(log_floor=-1.0), b"log_floor"),
                     (dict(log_floor=float("nan")), b"log_floor"), (dict(log_floor=float("inf")), b"log_floor")):
        c = pkg.ProsodyContour(cr.CONTOURS["step"], **kw)
        for entry in single.values():
            bad(entry(C.byref(c)), word)
        for entry in array.values():
            bad(entry(arr(c)), word, b"utterance 1")
    for points, word in (([], b"n_points"), ([(0.5, 2.0, 1.0, 1.0)] * 65, b"n_points")):
        c = pkg.ProsodyContour(points)
        for entry in single.values():
            bad(entry(C.byref(c)), word)
    # the frame count: 1 and 16385 with a contour that is not the identity (the entries that know F before a device is touched)
    big = np.zeros((513, 1), np.float32)
    for F in (1, 16385):
        bad(single["table"](C.byref(good), F), b"n_frames")
        bad(lib.xdtts_griffinlim_contour_linear(None, ptr(big), F, C.byref(good), ptr(out), C.byref(nf)), b"n_frames")
    bad(single["infer"](C.byref(good), 16385), b"n_frames")
    n2b = (C.c_size_t * 2)(3, 16385)
    bad(lib.xdtts_griffinlim_contour_linear_batch(None, S2, n2b, 2, arr(good), O2, nf2), b"n_frames", b"utterance 1")
    bad(lib.xdtts_griffinlim_contour_linear_batch(None, S2, (C.c_size_t * 2)(1, 3), 2, arr(good), O2, nf2), b"n_frames", b"utterance 0")
    # ... while the identity passes one frame and many: the next complaint is the null handle
    ident = pkg.ProsodyContour(cr.IDENTITY)
    for F in (1, 100000):
        bad(lib.xdtts_griffinlim_contour_linear(None, ptr(big), F, C.byref(ident), ptr(out), C.byref(nf)), b"null")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_contour_table_driver(tmp_path):
    """tests/contour_table_test.cpp with plain g++: the header at its limits (64 points, F = 16384 at rate 0.25, duplicate
    positions at 0 and 1) and every rule."""
    exe = str(tmp_path / "contour_table_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "contour_table_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_contour_header_needs_no_hip_and_is_the_one_implementation():
    src = open(os.path.join(CSRC, "prosody_contour.h"), encoding="utf-8").read()
    assert not re.search(r"#\s*include\s*\"", src)  # none of the library's headers
    assert not re.search(r"#\s*include\s*<hip/", src)
    assert not re.search(r"\b(hip[A-Z]\w*|__device__|__global__|__host__)\b", src)
    for name in os.listdir(CSRC):
        if name != "prosody_contour.h":
            text = open(os.path.join(CSRC, name), encoding="utf-8", errors="replace").read()
            assert not re.search(r"\binline size_t contour_fill\(|\bstruct ContourTable\b|65536\.0\s*/", text), name


# ---- the numpy restatement is itself right ------------------------------------------------------------------------------------


def test_reference_rate_step_moves_a_marker_to_where_the_table_says():
    """Rate 2 then 0.5 at pos 0.5 on 37 frames: a loud marker at input frame 20 appears at output frame c[20] / 65536 = 13, and
    F' = 46."""
    points = [(0.0, 2.0, 1.0, 1.0), (0.5, 2.0, 1.0, 1.0), (0.5, 0.5, 1.0, 1.0)]
    S = np.full((513, 37), 0.01, dtype=np.float32)
    S[:, 20] = 5.0
    c, _, _ = cr.table(points, 37)
    assert int(c[20]) % 65536 == 0 and int(c[20]) // 65536 == 13 and cr.frames(points, 37) == 46
    for dtype in (np.float64, np.float32):
        out, copied = cr.contour(S, points, dtype=dtype)
        assert out.shape == (513, 46) and out.dtype == dtype and copied.all()
        assert int(np.argmax(out[0])) == 13 and np.array_equal(out[:, 13], S[:, 20].astype(dtype))
    step = cr.CONTOURS["step"]  # the same warp with a pitch step: the marker is still loudest at frame 13
    out, copied = cr.contour(S, step)
    assert out.shape == (513, 46) and not copied.any() and int(np.argmax(out.sum(axis=0))) == 13


def test_reference_gain_zero_mutes_its_span_and_nothing_else():
    S = np.exp(np.random.default_rng(3).uniform(-9.0, 0.0, size=(513, 37))).astype(np.float32)  # no zero in the input
    for dtype in (np.float64, np.float32):
        out, copied = cr.contour(S, cr.CONTOURS["mute"], dtype=dtype)
        c, _, gain = cr.table(cr.CONTOURS["mute"], 37)
        assert copied.all() and np.all(gain[18:] == 0) and np.all(gain[:18] > 0)
        zero = np.all(out == 0, axis=0)
        assert np.array_equal(np.any(out == 0, axis=0), zero)  # a frame is muted whole or not at all
        first = int(np.argmax(zero))
        assert zero[first:].all() and not zero[:first].any() and 0 < first < out.shape[1] - 1
        assert first == -(-int(c[18]) // 65536) == 18  # the first output frame at or behind input frame 18, where the gain reaches 0


def test_reference_identity_and_float32_restatement():
    X = pr.random_magnitude(5, seed=5)
    out, copied = cr.contour(X, cr.IDENTITY)
    assert np.array_equal(out, X.astype(np.float64)) and copied.all()
    for name, points in cr.CONTOURS.items():
        r64, b64 = cr.contour(X, points)
        r32, b32 = cr.contour(X, points, dtype=np.float32)
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == r64.shape == (513, cr.frames(points, 5))
        assert np.array_equal(b64, b32) and pr.rel_err(r32, r64) < 2e-3, name
    # a rate-1 contour with pitch 1 and gain 1 on a span leaves that span's frames as they are
    half = [(0.0, 1.0, 1.0, 1.0), (0.5, 1.0, 1.0, 1.0), (0.5, 1.0, 1.25, 1.0)]
    X = pr.random_magnitude(9, seed=6)
    out, copied = cr.contour(X, half, dtype=np.float32)
    assert copied[:4].all() and not copied[4:].any() and np.array_equal(out[:, :4], X[:, :4])
