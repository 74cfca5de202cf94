"""CPU-only checks of the vocoder's analysis entries (audio -> magnitude -> mel, spectral convergence): declared, exported,
the frame count, and argument errors that come back as status codes before any device is touched."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xdtts_griffinlim_analysis_frames", "xdtts_griffinlim_analyze", "xdtts_griffinlim_analyze_batch",
       "xdtts_griffinlim_spectral_convergence", "xdtts_griffinlim_analysis_timings")


def test_analysis_symbols_are_declared_bound_and_exported(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdtts.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), "include/xdtts.h does not declare %s" % name
        assert name in pkg.SYMBOLS and hasattr(raw, name), name
    for method in ("analyze", "analyze_batch", "spectral_convergence", "analysis_timings", "analysis_frames"):
        assert callable(getattr(pkg.GriffinLim, method))


def test_analysis_frames_is_n_over_hop_plus_one(pkg):
    """n_frames = n_samples / 256 + 1 (librosa.stft, center=True) -- host arithmetic, no handle needed."""
    for n in (1, 255, 256, 1000, 9216):
        assert pkg.lib.xdtts_griffinlim_analysis_frames(None, n) == n // 256 + 1, n
    assert pkg.lib.xdtts_griffinlim_analysis_frames(None, 256 * 39) == 40  # the audio of a 40-frame mel analyses to 40 frames


def test_analysis_entries_reject_bad_arguments_without_touching_a_device(pkg):
    """Null pointers, no samples, no utterances: XDTTS_ERR_BAD_ARG with a message, before anything is launched -- so this runs
    without a GPU too (no handle can exist there: the handle argument is the null one)."""
    lib = pkg.lib
    y = np.zeros(512, dtype=np.float32)
    S = np.ones((513, 3), dtype=np.float32)
    mel = np.zeros((80, 3), dtype=np.float32)
    nf = C.c_size_t()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def bad(st, word):
        assert st == pkg.XDTTS_ERR_BAD_ARG
        assert word in lib.xdtts_last_error(), lib.xdtts_last_error()

    bad(lib.xdtts_griffinlim_analyze(None, p(y), y.size, 1e-5, p(S), p(mel), C.byref(nf)), b"null")
    bad(lib.xdtts_griffinlim_analyze(None, None, 0, 0.0, None, None, None), b"null")
    ptrs = (C.c_void_p * 1)(y.ctypes.data)
    ns = (C.c_size_t * 1)(y.size)
    bad(lib.xdtts_griffinlim_analyze_batch(None, ptrs, ns, 1, 1e-5, None, None, None), b"null")
    bad(lib.xdtts_griffinlim_analyze_batch(None, None, None, 0, 1e-5, None, None, None), b"null")
    out = (C.c_float * 2)()
    bad(lib.xdtts_griffinlim_spectral_convergence(None, p(y), y.size, p(S), 3, 0, C.byref(out)), b"null")
    bad(lib.xdtts_griffinlim_spectral_convergence(None, None, 0, None, 0, 0, None), b"null")
    ms = (C.c_float * 3)()
    bad(lib.xdtts_griffinlim_analysis_timings(None, C.byref(ms)), b"null")
    bad(lib.xdtts_griffinlim_analysis_timings(None, None), b"null")
