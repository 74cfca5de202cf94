"""Pitch tracker and pitch targets (xdtts_f0_opts, xdtts_pitch_target) without a GPU: the argument rules, the quefrency range,
the host reference of the utterance stage against the numpy restatement (tests/f0_ref.py), the plain-C++ driver of f0_plan.h,
and the accuracy of the definition itself -- conditions on the fp64 restatement, on synthetic voiced sounds and on noise."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contour_ref as cr
import f0_ref as fr
import prosody_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = [
    "xdtts_f0_opts_default", "xdtts_pitch_target_default", "xdtts_f0_plan", "xdtts_f0_track_reference",
    "xdtts_griffinlim_f0_linear", "xdtts_griffinlim_f0_linear_batch", "xdtts_griffinlim_f0", "xdtts_griffinlim_f0_audio",
    "xdtts_griffinlim_pitch_target_linear", "xdtts_griffinlim_pitch_target_linear_batch",
    "xdtts_griffinlim_infer_pitch_target", "xdtts_griffinlim_infer_batch_pitch_target",
    "xdtts_synthesize_ids_pitch_target", "xdtts_synthesize_batch_pitch_target", "xdtts_griffinlim_last_f0",
]
FRAMES = [1, 2, 5, 6, 37, 64]
TARGETS = [(0, 1.0, 1.0), (1, 180.0, 1.0), (2, 1.1, 0.5), (2, 1.0, 0.0), (2, 1.0, 2.0), (1, 400.0, 4.0), (1, 60.0, 0.0), (2, 0.5, 4.0)]


def test_f0_symbols_are_declared_bound_exported_and_mirrored(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdtts.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.LIB_PATH)
    host = open(os.path.join(ROOT, "include", "xdtts_host.hpp")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), "include/xdtts.h does not declare %s" % name
        assert name in pkg.SYMBOLS and hasattr(raw, name), name
        assert name in host, "include/xdtts_host.hpp does not mirror %s" % name
    assert C.sizeof(pkg.F0Opts) == 20 and C.sizeof(pkg.PitchTarget) == 12 and C.sizeof(pkg.F0Stats) == 28
    o, t = pkg.F0Opts(), pkg.PitchTarget()
    assert (o.fmin, o.fmax, o.octave_bias) == (60.0, 400.0, np.float32(0.9)) and o.threshold == np.float32(0.2) and o.log_floor == np.float32(1e-5)
    assert (t.mode, t.value, t.range) == (0, 1.0, 1.0)
    for fn in (pkg.synthesize, pkg.synthesize_batch):
        assert "target" in fn.__code__.co_varnames and "f0_opts" in fn.__code__.co_varnames


def test_quefrency_range(pkg):
    assert pkg.f0_plan() == fr.plan() == (56, 367)
    assert pkg.f0_plan(pkg.F0Opts(fmin=50.0, fmax=1000.0)) == fr.plan(50.0, 1000.0) == (23, 441)
    with pytest.raises(pkg.XdttsError) as e:  # q_lo == q_hi == 441
        pkg.f0_plan(pkg.F0Opts(fmin=50.0, fmax=50.1))
    assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and "fmin" in str(e.value) and "fmax" in str(e.value)
    assert fr.plan(50.0, 50.1) == (441, 441) and not fr.opts_ok(fr.opts(fmin=50.0, fmax=50.1))


BAD_OPTS = [("fmin", 49.9), ("fmin", float("nan")), ("fmin", 400.0), ("fmin", 500.0), ("fmax", 1000.5), ("fmax", float("inf")),
            ("threshold", -0.1), ("threshold", float("nan")), ("octave_bias", 0.0), ("octave_bias", 1.01), ("octave_bias", float("nan")),
            ("log_floor", 0.0), ("log_floor", -1.0), ("log_floor", float("inf"))]
BAD_TARGETS = [("mode", dict(mode=3)), ("mode", dict(mode=-1)), ("value", dict(mode=1, value=49.0)), ("value", dict(mode=1, value=1001.0)),
               ("value", dict(mode=1, value=float("nan"))), ("value", dict(mode=2, value=0.49)), ("value", dict(mode=2, value=2.01)),
               ("range", dict(range=-0.1)), ("range", dict(range=4.1)), ("range", dict(range=float("nan")))]


def test_rules_of_opts_and_target_agree_with_the_restatement(pkg):
    for field, v in BAD_OPTS:
        assert not fr.opts_ok(fr.opts(**{field: v}))
    assert fr.opts_ok(fr.opts()) and fr.opts_ok(fr.opts(fmin=50.0, fmax=1000.0, threshold=0.0, octave_bias=1.0))
    for _, kw in BAD_TARGETS:
        t = dict(mode=0, value=1.0, range=1.0)
        t.update(kw)
        assert not fr.target_ok(t["mode"], t["value"], t["range"])
    assert fr.target_ok(0, float("nan"), 1.0)  # mode 0 ignores the value
    for mode, value, rng in TARGETS:
        assert fr.target_ok(mode, value, rng)


def test_entries_reject_bad_arguments_without_touching_a_device(pkg):
    """Every rule: XDTTS_ERR_BAD_ARG and the field's name in the message, on null handles through each entry -- nothing is
    launched, so this runs without a GPU.  The array entries name the utterance and clear their outputs."""
    lib = pkg.lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    S, out, mel = np.ones((513, 3), np.float32), np.zeros((513, 3), np.float32), np.zeros((80, 3), np.float32)
    raw = np.full(3, 100.0, np.float32)
    ids, lens, uc = np.array([[64, 65, 7], [64, 65, 7]], dtype=np.int64), np.array([3, 3], np.int32), np.array([1, 1], np.int32)
    nf, ns = C.c_size_t(7), C.c_size_t(7)
    audio, melp = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
    S2, M2, n2 = (C.c_void_p * 2)(S.ctypes.data, S.ctypes.data), (C.c_void_p * 2)(mel.ctypes.data, mel.ctypes.data), (C.c_size_t * 2)(3, 3)
    good_t = pkg.PitchTarget(hz=180.0)

    def tarr(t):
        a = (pkg.PitchTarget * 2)()
        for u, x in enumerate((good_t, t)):
            a[u].mode, a[u].value, a[u].range = x.mode, x.value, x.range
        return a

    def entries(o_obj, t_obj):
        o, t = (None if o_obj is None else C.byref(o_obj)), C.byref(t_obj)
        tarr2 = tarr(t_obj)
        outs2, ns2, nf2 = (C.POINTER(C.c_float) * 2)(), (C.c_size_t * 2)(5, 5), (C.c_size_t * 2)(5, 5)
        mels2 = (C.POINTER(C.c_float) * 2)()
        return {
            "reference": lambda: lib.xdtts_f0_track_reference(ptr(raw), ptr(raw), 3, o, t, None, None, None),
            "linear": lambda: lib.xdtts_griffinlim_pitch_target_linear(None, ptr(S), 3, o, t, None, ptr(out), None, None),
            "linear_batch": lambda: lib.xdtts_griffinlim_pitch_target_linear_batch(None, S2, n2, 2, o, tarr2, None, None, None, None),
            "infer": lambda: lib.xdtts_griffinlim_infer_pitch_target(None, ptr(mel), 80, 3, o, t, None, C.byref(audio), C.byref(ns)),
            "infer_batch": lambda: (lib.xdtts_griffinlim_infer_batch_pitch_target(None, M2, 80, n2, 2, o, tarr2, None, outs2, ns2), list(ns2)),
            "synth": lambda: lib.xdtts_synthesize_ids_pitch_target(None, None, ptr(ids), 3, None, 0, None, o, t, None, C.byref(melp), C.byref(nf), C.byref(audio), C.byref(ns)),
            "synth_batch": lambda: (lib.xdtts_synthesize_batch_pitch_target(None, None, ptr(ids), ptr(lens), 2, 3, ptr(uc), 2, None, None, o, tarr2, None, mels2, nf2, outs2, ns2), list(ns2) + list(nf2)),
        }

    def status_of(r):
        return r[0] if isinstance(r, tuple) else r

    tracker_only = {
        "plan": lambda o: lib.xdtts_f0_plan(o, None, None),
        "f0_linear": lambda o: lib.xdtts_griffinlim_f0_linear(None, ptr(S), 3, o, None, None, None, None),
        "f0_linear_batch": lambda o: lib.xdtts_griffinlim_f0_linear_batch(None, S2, n2, 2, o, None, None, None, None),
        "f0": lambda o: lib.xdtts_griffinlim_f0(None, ptr(mel), 80, 3, o, None, None, None, None),
        "f0_audio": lambda o: lib.xdtts_griffinlim_f0_audio(None, ptr(raw), 3, o, None, None, None, None),
    }
    for field, v in BAD_OPTS:
        o = pkg.F0Opts(**{field: v})
        for name, call in list(entries(o, good_t).items()) + [(k, (lambda f=f: f(C.byref(o)))) for k, f in tracker_only.items()]:
            r = call()
            assert status_of(r) == pkg.XDTTS_ERR_BAD_ARG, (name, field, v)
            msg = pkg.lib.xdtts_last_error().decode()
            assert field in msg or ("fmin" in msg and field == "fmax"), (name, field, v, msg)
            if isinstance(r, tuple):
                assert not any(r[1]), (name, "outputs cleared")
    for field, kw in BAD_TARGETS:
        t = pkg.PitchTarget(**kw)
        for name, call in entries(None, t).items():
            r = call()
            assert status_of(r) == pkg.XDTTS_ERR_BAD_ARG, (name, field, kw)
            msg = pkg.lib.xdtts_last_error().decode()
            assert field in msg, (name, field, msg)
            if name in ("linear_batch", "infer_batch", "synth_batch"):
                assert "utterance 1" in msg, (name, msg)
    # a good request gets as far as the handle
    for name, call in entries(None, good_t).items():
        assert status_of(call()) == (0 if name == "reference" else pkg.XDTTS_ERR_BAD_ARG), name


def _cases(F, seed):
    """(raw, strength) inputs of the utterance stage: all voiced, none voiced, alternating, one outlier at twice the value, and
    many equal values (ties in the selection)."""
    rng = np.random.default_rng(seed)
    smooth = (140.0 * np.exp2(0.05 * np.sin(np.arange(F) / 3.0) + 0.004 * rng.standard_normal(F))).astype(np.float32)
    strong = rng.uniform(0.25, 0.6, F).astype(np.float32)
    out = {
        "all": (smooth, strong),
        "none": (smooth, np.full(F, 0.1, np.float32)),
        "alternating": (smooth, np.where(np.arange(F) % 2 == 0, strong, np.float32(0.05)).astype(np.float32)),
        "ties": (np.where(rng.random(F) < 0.7, np.float32(123.25), np.float32(150.5)).astype(np.float32), strong),
    }
    outlier = smooth.copy()
    outlier[F // 2] *= 2
    out["outlier"] = (outlier, strong)
    nan_strength = strong.copy()
    nan_strength[0] = np.nan
    out["nan"] = (smooth, nan_strength)
    return out


def ulp_distance(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.all(a > 0) and np.all(b > 0)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_against_restatement(pkg, raw, strength, target, f0, ratio, stats, what):
    """f0, voiced flags and every stats field bit for bit; ratio within 2 ulp of the fp32 restatement."""
    rf0, voiced, rratio, rs = fr.track(raw, strength, fr.opts(), target, np.float32)
    assert np.array_equal(f0.view(np.uint32), rf0.view(np.uint32)), what
    assert np.array_equal(f0 > 0, voiced), what
    got = dict(zip(("n_frames", "n_voiced", "n_clamped", "median_hz", "min_hz", "max_hz", "base_ratio"), stats.astuple()))
    for k in ("n_frames", "n_voiced", "n_clamped"):
        assert got[k] == rs[k], (what, k, got[k], rs[k])
    for k in ("median_hz", "min_hz", "max_hz", "base_ratio"):
        assert np.float32(got[k]).view(np.uint32) == np.float32(rs[k]).view(np.uint32), (what, k, got[k], rs[k])
    assert ulp_distance(ratio, rratio).max() <= 2, (what, ulp_distance(ratio, rratio).max())
    assert np.all(ratio >= 0.5) and np.all(ratio <= 2.0)


@pytest.mark.parametrize("F", FRAMES)
def test_reference_equals_the_numpy_restatement(pkg, F):
    for name, (raw, strength) in _cases(F, seed=F).items():
        for target in TARGETS:
            f0, ratio, stats = pkg.f0_track_reference(raw, strength, target=pkg.PitchTarget(mode=target[0], value=target[1], range=target[2]))
            check_against_restatement(pkg, raw, strength, target, f0, ratio, stats, (name, F, target))
            if name == "none":
                assert stats.n_voiced == 0 and stats.base_ratio == 1.0 and np.all(ratio == 1.0) and np.all(f0 == 0)
            if name == "outlier" and F >= 5:  # the median of five removes a single octave error
                assert f0[F // 2] < 1.2 * 140.0
            if target == (2, 1.0, 0.0) and stats.n_voiced:
                # flattened: every voiced frame lands on the median, up to the two log2 roundings (half an ulp of 7.x = 2.4e-7
                # each, times ln 2 in the ratio) and the roundings of exp2 and of the product: 4.5e-7 in all
                assert np.allclose(f0[f0 > 0] * ratio[f0 > 0], stats.median_hz, rtol=1e-6, atol=0)


def test_reference_outputs_are_optional_and_the_identity_gives_ones(pkg):
    raw, strength = _cases(37, seed=1)["all"]
    assert pkg.lib.xdtts_f0_track_reference(raw.ctypes.data_as(C.c_void_p), strength.ctypes.data_as(C.c_void_p), 37, None, None, None, None, None) == 0
    for t in (pkg.PitchTarget(), pkg.PitchTarget(factor=1.0)):
        _, ratio, stats = pkg.f0_track_reference(raw, strength, target=t)
        assert np.all(ratio == 1.0) and stats.n_clamped == 0 and stats.base_ratio == 1.0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_f0_plan_driver(tmp_path):
    """tests/f0_plan_test.cpp with plain g++: the header at its limits (F = 16384, range 0 and 4 with the clamp engaging,
    no voiced frame) and every rule; and once more as a stand-alone program under the address and undefined-behaviour sanitizers."""
    src = os.path.join(ROOT, "tests", "f0_plan_test.cpp")
    exe = str(tmp_path / "f0_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]
    san = str(tmp_path / "f0_plan_test_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, src, "-o", san])
    assert subprocess.check_output([san]).decode().split() == ["ok"]


def test_f0_header_needs_no_hip():
    src = open(os.path.join(CSRC, "f0_plan.h"), encoding="utf-8").read()
    assert not re.search(r"#\s*include\s*\"", src)  # none of the library's headers
    assert "hip/" not in src


# ---- the accuracy of the definition: conditions on the fp64 restatement ----
@pytest.fixture(scope="module")
def voiced_cases(pkg):
    """{(f0, kind): S (513, 64)}: voiced_signal(256 * 63, f0, vibrato 0.03), its true magnitude and the same through the mel basis."""
    import gpu_f0_cases as gc

    return gc.voiced_magnitudes(pkg)


def measure(S, f0_true):
    """(f0 [F], voiced [F]) of the fp64 restatement at threshold 0.2, and the checks the issue sets on frames 4 .. F - 5."""
    _, raw, strength, _ = fr.frames(S, fr.opts(), np.float64)
    f0, voiced, _, stats = fr.track(raw.astype(np.float32), strength.astype(np.float32), fr.opts())
    return f0, voiced, stats


@pytest.mark.parametrize("f0,kind", [(140.0, "true"), (140.0, "mel"), (220.0, "true"), (220.0, "mel")])
def test_reference_tracks_a_voiced_sound(voiced_cases, f0, kind):
    S = voiced_cases[(f0, kind)]
    F = S.shape[1]
    est, voiced, _ = measure(S, f0)
    inner = slice(4, F - 4)  # frames 4 .. F - 5
    assert voiced[inner].mean() >= 0.9, voiced[inner].mean()
    err = np.abs(fr.cents(est[inner][voiced[inner]], fr.true_f0(F, f0)[inner][voiced[inner]]))
    print("tracking %s %g Hz: voiced %.3f, max %.1f cents, rms %.1f cents" % (kind, f0, voiced[inner].mean(), err.max(), np.sqrt(np.mean(err ** 2))))
    assert err.max() <= 30.0, err.max()


@pytest.mark.parametrize("f0,kind", [(140.0, "true"), (140.0, "mel"), (220.0, "true"), (220.0, "mel")])
def test_reference_targets_move_the_median_and_scale_the_range(voiced_cases, f0, kind):
    S = voiced_cases[(f0, kind)]
    F = S.shape[1]
    est, voiced, _ = measure(S, f0)
    e_in = fr.excursion_cents(est, voiced)
    for k in (0.85, 1.15):
        out, _, _, _ = fr.pitch_target(S, (1, k * f0, 1.0))
        e2, v2, st2 = measure(out, f0)
        med = fr.lower_median(e2[4 : F - 4][v2[4 : F - 4]])
        print("target %s %g Hz x %.2f: median %.2f Hz (%.2f %%)" % (kind, f0, k, med, 100 * (med / (k * f0) - 1)))
        assert abs(med / (k * f0) - 1.0) <= 0.01, (k, med)
    out, _, _, _ = fr.pitch_target(S, (2, 1.0, 0.0))
    e0, v0, _ = measure(out, f0)
    out, _, _, _ = fr.pitch_target(S, (2, 1.0, 2.0))
    e2, v2, _ = measure(out, f0)
    x0, x2 = fr.excursion_cents(e0, v0), fr.excursion_cents(e2, v2)
    print("range %s %g Hz: input %.1f cents, range 0 -> %.1f, range 2 -> %.1f (x %.2f)" % (kind, f0, e_in, x0, x2, x2 / e_in))
    assert x0 <= e_in / 3.0, (x0, e_in)
    assert 1.7 * e_in <= x2 <= 2.4 * e_in, (x2, e_in)


def test_reference_finds_no_voice_in_white_noise():
    y = 0.1 * np.random.default_rng(1).standard_normal(256 * 47)
    S = pr.stft_magnitude(y).astype(np.float32)
    _, _, strength, _ = fr.frames(S, fr.opts(), np.float64)
    print("white noise: largest cepstral strength %.3f" % strength.max())
    assert not np.any(strength >= 0.2)


def test_float32_restatement_stays_inside_the_gpu_tests_cap(voiced_cases):
    """The seeds of tests/test_gpu_f0.py, checked here: on each of its magnitudes the fp32 restatement alone disagrees with the
    fp64 n* on at most 2 % of the frames, and only where the fp64 cepstrum is ambiguous within the bound."""
    import gpu_f0_cases as gc

    for name, S in gc.frame_cases(voiced_cases).items():
        n64, raw64, s64, c64 = fr.frames(S, fr.opts(), np.float64)
        n32, raw32, s32, c32 = fr.frames(S, fr.opts(), np.float32)
        d32 = float(np.max(np.abs(c32[:, :513].astype(np.float64) - c64[:, :513])))
        bound = 4 * d32 + 2e-5
        differ = n64 != n32
        amb = fr.ambiguous(c64, fr.opts(), bound)
        assert not np.any(differ & ~amb), name
        assert differ.sum() <= 0.02 * S.shape[1], (name, int(differ.sum()), S.shape[1])
