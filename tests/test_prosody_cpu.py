"""CPU-only checks of the prosody entries (speaking rate and pitch in the vocoder): declared, bound and exported, the defaults,
the frame count, argument errors that come back as status codes before any device is touched -- and the numpy restatement of
the definition (tests/prosody_ref.py), which the GPU tests take as their reference, doing what the definition promises."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prosody_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xdtts_prosody_default", "xdtts_prosody_frames", "xdtts_griffinlim_prosody_linear", "xdtts_griffinlim_infer_prosody",
       "xdtts_synthesize_ids_prosody")


def test_prosody_symbols_are_declared_bound_and_exported(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdtts.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), "include/xdtts.h does not declare %s" % name
        assert name in pkg.SYMBOLS and hasattr(raw, name), name
    assert re.search(r"typedef\s+struct\s*\{[^}]*\bfloat\s+rate;[^}]*\bfloat\s+pitch;[^}]*\bint32_t\s+lifter;[^}]*\bfloat\s+log_floor;[^}]*\}\s*xdtts_prosody;", text)
    for method in ("prosody_linear", "infer_prosody"):
        assert callable(getattr(pkg.GriffinLim, method))
    assert "prosody" in pkg.synthesize.__code__.co_varnames
    host = open(os.path.join(ROOT, "include", "xdtts_host.hpp")).read()
    for name in ("xdtts_griffinlim_prosody_linear", "xdtts_griffinlim_infer_prosody", "xdtts_synthesize_ids_prosody", "xdtts_prosody_frames"):
        assert name in host, "include/xdtts_host.hpp does not mirror %s" % name


def test_prosody_default_is_the_identity_with_a_30_bin_lifter(pkg):
    p = pkg.Prosody()
    p.rate, p.pitch, p.lifter, p.log_floor = 9.0, 9.0, 9, 9.0
    pkg.lib.xdtts_prosody_default(C.byref(p))
    assert (p.rate, p.pitch, p.lifter, p.log_floor) == (1.0, 1.0, 30, float(np.float32(1e-5)))
    pkg.lib.xdtts_prosody_default(None)  # a null pointer is ignored
    q = pkg.Prosody(rate=1.25, lifter=40)
    assert (q.rate, q.pitch, q.lifter) == (1.25, 1.0, 40)
    assert C.sizeof(pkg.Prosody) == 16


@pytest.mark.parametrize("F, rate, want", [(2, 4.0, None), (2, 0.25, None), (5, 1.25, 4), (48, 0.7, 68), (800, 1.25, 640), (800, 1.0, 800)])
def test_prosody_frames_is_the_formula(pkg, F, rate, want):
    """F' = F at rate 1, else max(floor((F - 1) / rate + 0.5), 1) + 1, written out here independently of prosody_ref."""
    r = float(np.float32(rate))
    formula = F if r == 1.0 else max(int(np.floor((F - 1) / r + 0.5)), 1) + 1
    got = pkg.lib.xdtts_prosody_frames(F, rate)
    assert got == formula == pr.prosody_frames(F, rate) == pkg.prosody_frames(F, rate), (got, formula)
    if want is not None:
        assert got == want
    assert got >= 2 or r == 1.0


def test_prosody_frames_is_zero_for_a_bad_argument(pkg):
    f = pkg.lib.xdtts_prosody_frames
    for rate in (0.0, 5.0, float("nan"), float("inf"), -1.0, 0.2499, 4.001):
        assert f(100, rate) == 0, rate
    assert f(1, 1.25) == 0 and f(0, 0.5) == 0  # F < 2 at rate != 1
    assert f(1, 1.0) == 1 and f(0, 1.0) == 0   # the identity passes the count through


def test_prosody_entries_reject_bad_arguments_without_touching_a_device(pkg):
    """Null pointers and each out-of-range field: XDTTS_ERR_BAD_ARG with a message, on the null handle -- nothing is launched, so
    this runs without a GPU too."""
    lib = pkg.lib
    S = np.ones((513, 3), dtype=np.float32)
    out = np.zeros((513, 12), dtype=np.float32)
    mel = np.zeros((80, 3), dtype=np.float32)
    ids = np.array([64, 65, 7], dtype=np.int64)
    nf, ns = C.c_size_t(), C.c_size_t()
    audio, melp = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = pkg.Prosody(rate=1.25, pitch=0.8)

    def linear(p, S_=S, out_=out):
        return lib.xdtts_griffinlim_prosody_linear(None, None if S_ is None else ptr(S_), 3, p, None if out_ is None else ptr(out_), C.byref(nf))

    def infer(p, mel_=mel, audio_=C.byref(audio)):
        return lib.xdtts_griffinlim_infer_prosody(None, None if mel_ is None else ptr(mel_), 80, 3, p, audio_, C.byref(ns))

    def synth(p):
        return lib.xdtts_synthesize_ids_prosody(None, None, ptr(ids), ids.size, None, 0, None, p, C.byref(melp), C.byref(nf), C.byref(audio), C.byref(ns))

    def bad(st, word):
        assert st == pkg.XDTTS_ERR_BAD_ARG, st
        assert word in lib.xdtts_last_error(), lib.xdtts_last_error()

    for entry in (linear, infer, synth):
        bad(entry(C.byref(good)), b"null")  # the null handle
        bad(entry(None), b"null")           # the null prosody
    bad(linear(C.byref(good), S_=None), b"null")
    bad(linear(C.byref(good), out_=None), b"null")
    bad(infer(C.byref(good), mel_=None), b"null")
    bad(infer(C.byref(good), audio_=None), b"null")
    # each field out of range, through the entry that checks the prosody before anything else
    for kw, word in ((dict(rate=0.2), b"rate"), (dict(rate=4.5), b"rate"), (dict(rate=float("nan")), b"rate"), (dict(rate=float("inf")), b"rate"),
                     (dict(pitch=0.4), b"pitch"), (dict(pitch=2.5), b"pitch"), (dict(pitch=float("nan")), b"pitch"),
                     (dict(lifter=0), b"lifter"), (dict(lifter=256), b"lifter"),
                     (dict(log_floor=0.0), b"log_floor"), (dict(log_floor=-1.0), b"log_floor"), (dict(log_floor=float("nan")), b"log_floor"),
                     (dict(log_floor=float("inf")), b"log_floor")):
        bad(synth(C.byref(pkg.Prosody(**kw))), word)


# ---- the numpy restatement is itself right ------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def voiced():
    S = pr.stft_magnitude(pr.voiced_signal()).astype(np.float32)  # the true magnitude, F = 48
    S.setflags(write=False)
    return S, float(np.median(pr.cepstral_peak(S)))


def test_the_voiced_signal_has_its_pitch_period_where_it_should(voiced):
    S, q_in = voiced
    assert S.shape == (513, 48) and abs(q_in - pr.SR / 140.0) <= 2.0, q_in  # 157.5 samples


@pytest.mark.parametrize("pitch", [0.75, 0.8, 1.25, 1.5])
def test_reference_moves_the_cepstral_pitch_peak(voiced, pitch):
    """On the true magnitude the median cepstral peak of S' lies within 2 samples of q_in / pitch (measured: within 0.6; the
    two samples are the integer argmax at both ends)."""
    S, q_in = voiced
    Sp = pr.prosody(S, 1.0, pitch)
    q = float(np.median(pr.cepstral_peak(Sp)))
    print("pitch %.2f: peak %.1f, q_in / pitch %.1f" % (pitch, q, q_in / pitch))
    assert Sp.shape == S.shape and np.all(np.isfinite(Sp)) and np.all(Sp > 0)
    assert abs(q - q_in / pitch) <= 2.0, (q, q_in / pitch)


def test_reference_rate_alone_keeps_the_peak_and_the_envelope_stays_put(voiced):
    S, q_in = voiced
    for rate in (1.25, 0.7):
        Sr = pr.prosody(S, rate, 1.0)
        assert Sr.shape == (513, pr.prosody_frames(48, rate))
        assert float(np.median(pr.cepstral_peak(Sr))) == q_in
    assert np.array_equal(pr.prosody(S, 1.0, 1.0), S.astype(np.float64))
    S2 = pr.prosody(S, 2.0, 1.0)  # u = 2 j: every second frame as it is, then the last one (u clamped to F - 1)
    assert S2.shape == (513, 25) and np.array_equal(S2[:, :24], S[:, 0:48:2]) and np.array_equal(S2[:, 24], S[:, 47])
    # the envelope (the low quefrencies of the log magnitude) is where it was: the formants do not move with the pitch
    def envelope(X):
        L = np.log(np.maximum(X.T.astype(np.float64), 1e-5))
        c = np.fft.irfft(L, n=1024, axis=1)
        c[:, 31:-30] = 0
        return np.fft.rfft(c, axis=1).real

    E0 = envelope(S)
    for pitch in (0.8, 1.25):
        d = np.abs(envelope(pr.prosody(S, 1.0, pitch)) - E0)
        print("pitch %.2f: envelope moved by %.3f nepers at most, %.4f in the mean" % (pitch, d.max(), d.mean()))
        assert d.mean() < 0.115, d.mean()  # under 1 dB (0.115 nepers) in the mean: the fine structure it sits under swings by several nepers


def test_reference_float32_restatement_stays_in_single_precision():
    X = pr.random_magnitude(5, seed=5)
    for rate, pitch in ((1.0, 1.3), (2.0, 2.0), (1.25, 1.0)):
        r32, r64 = pr.prosody(X, rate, pitch, dtype=np.float32), pr.prosody(X, rate, pitch)
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == r64.shape
        assert pr.rel_err(r32, r64) < 1e-3
    zeros = X == 0
    assert zeros.any() and np.array_equal(pr.prosody(X, 1.0, 1.0, dtype=np.float32) == 0, zeros)
