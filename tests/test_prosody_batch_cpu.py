"""CPU-only checks of the per-utterance prosody entries (batch, sequence and the ragged parity hook): declared, bound, exported
and mirrored, and the argument errors of the prosody ARRAY, which come back as status codes before a handle is looked at -- so
they are tried on null handles and need no GPU.  The ragged reference of the GPU tests is prosody_ref.prosody per utterance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xdtts_griffinlim_prosody_linear_batch", "xdtts_griffinlim_infer_batch_prosody", "xdtts_synthesize_batch_prosody",
       "xdtts_synthesize_sequence_prosody")


def test_the_four_entries_are_declared_bound_exported_and_mirrored(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdtts.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.LIB_PATH)
    host = open(os.path.join(ROOT, "include", "xdtts_host.hpp")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), "include/xdtts.h does not declare %s" % name
        assert name in pkg.SYMBOLS and hasattr(raw, name), name
        assert name in host, "include/xdtts_host.hpp does not mirror %s" % name
    assert callable(pkg.GriffinLim.prosody_linear_batch)
    for fn in (pkg.GriffinLim.infer_batch, pkg.synthesize_batch, pkg.synthesize_sequence):
        assert "prosody" in fn.__code__.co_varnames[: fn.__code__.co_argcount], fn.__name__
    assert "Out of scope: the batch and sequence entries" not in open(os.path.join(ROOT, "include", "xdtts.h")).read()


@pytest.fixture(scope="module")
def entries(pkg):
    """name -> call(prosody array or None, n_utt) on null handles, with every other argument in order for 3 utterances."""
    lib = pkg.lib
    n = 3
    keep = []

    def arr(ctype, vals):
        a = (ctype * n)(*vals)
        keep.append(a)
        return a

    S = [np.ones((513, 3), dtype=np.float32) for _ in range(n)]
    out = [np.zeros((513, 12), dtype=np.float32) for _ in range(n)]
    mel = [np.zeros((80, 3), dtype=np.float32) for _ in range(n)]
    ids = np.tile(np.array([64, 65, 7], dtype=np.int64), (n, 1))
    lens = np.full(n, 3, dtype=np.int32)
    chunks = np.ones(n, dtype=np.int32)
    keep += [S, out, mel, ids, lens, chunks]
    Sp, Op, Mp = (arr(C.c_void_p, [a.ctypes.data for a in x]) for x in (S, out, mel))
    idp = arr(C.c_void_p, [ids[u].ctypes.data for u in range(n)])
    nf = arr(C.c_size_t, [3] * n)
    nid = arr(C.c_size_t, [3] * n)
    o_mel, o_audio = (C.POINTER(C.c_float) * n)(), (C.POINTER(C.c_float) * n)()
    o_nf, o_ns = (C.c_size_t * n)(), (C.c_size_t * n)()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return {
        "linear_batch": lambda p, k: lib.xdtts_griffinlim_prosody_linear_batch(None, Sp, nf, k, p, Op, o_nf),
        "infer_batch": lambda p, k: lib.xdtts_griffinlim_infer_batch_prosody(None, Mp, 80, nf, k, p, o_audio, o_ns),
        "synthesize_batch": lambda p, k: lib.xdtts_synthesize_batch_prosody(None, None, ptr(ids), ptr(lens), k, 3, ptr(chunks), k, None, None, p, o_mel, o_nf, o_audio, o_ns),
        "synthesize_sequence": lambda p, k: lib.xdtts_synthesize_sequence_prosody(None, None, idp, nid, None, None, k, None, p, o_mel, o_nf, o_audio, o_ns),
    }


NAMES = ("linear_batch", "infer_batch", "synthesize_batch", "synthesize_sequence")


def bad(pkg, st, *words):
    msg = pkg.lib.xdtts_last_error()
    assert st == pkg.XDTTS_ERR_BAD_ARG, (st, msg)
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("name", NAMES)
def test_null_array_and_no_utterance_are_bad_arguments(pkg, entries, name):
    good = (pkg.Prosody * 3)(pkg.Prosody(rate=1.25), pkg.Prosody(), pkg.Prosody(pitch=0.8))
    bad(pkg, entries[name](None, 3), b"null prosody")
    bad(pkg, entries[name](good, 0), b"at least one utterance")
    bad(pkg, entries[name](good, 3))  # the array is fine: the null handle is what is left to complain about
    assert b"prosody" not in pkg.lib.xdtts_last_error()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kw, word", [(dict(rate=4.5), b"rate"), (dict(pitch=0.4), b"pitch"), (dict(lifter=256), b"lifter"),
                                      (dict(log_floor=0.0), b"log_floor"), (dict(rate=float("nan")), b"rate"),
                                      (dict(pitch=float("nan")), b"pitch")])
def test_a_bad_field_in_element_2_is_named_with_its_index(pkg, entries, name, kw, word):
    ps = (pkg.Prosody * 3)(pkg.Prosody(rate=1.25), pkg.Prosody(), pkg.Prosody(**kw))
    bad(pkg, entries[name](ps, 3), word, b"utterance 2")
