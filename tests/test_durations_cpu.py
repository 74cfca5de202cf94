"""The durations stage without a device (include/xdtts.h; csrc/durations_plan.h): the bindings and structs, the argument rules
(before any handle), the numpy restatement (tests/durations_ref.py) against the library's host reference bit for bit, the two
maps, the sanitizer-built stand-alone driver of the plan header -- and the discrimination of the GPU test's bound: on the GPU
test's own inputs, from the fp64 oracle, every plausible mistake of the stage moves at least one id by 100 bounds."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import durations_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ["xdtts_durations_default", "xdtts_tacotron2_set_durations", "xdtts_tacotron2_get_durations", "xdtts_tacotron2_last_durations_count",
       "xdtts_tacotron2_last_durations", "xdtts_tacotron2_last_alignment", "xdtts_tacotron2_durations_gather", "xdtts_durations_reference",
       "xdtts_durations_position", "xdtts_durations_samples"]

BOUND_CAP = dr.BOUND_CAP
assert_same = dr.assert_same


def test_symbols_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "xdtts.h")).read()
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in pkg.SYMBOLS, name
    for attr in ("set_durations", "get_durations", "last_durations", "last_alignment", "last_durations_count", "durations_gather"):
        assert callable(getattr(pkg.Tacotron2, attr))


def test_structs_and_default(pkg):
    assert C.sizeof(pkg.DurationsOpts) == 12 and C.sizeof(pkg.AlignmentStats) == 48
    o = pkg.DurationsOpts()
    assert (o.on, o.min_frames, o.max_frames) == (0, 0.5, 40.0)
    assert tuple(f[0] for f in pkg.AlignmentStats._fields_) == dr.STATS_FIELDS
    pkg.lib.xdtts_durations_default(None)  # a null pointer is ignored


def test_argument_errors_come_before_a_handle(pkg):
    for field, kw in (("on", dict(on=2)), ("min_frames", dict(min_frames=-1.0)), ("min_frames", dict(min_frames=float("nan"))),
                      ("max_frames", dict(max_frames=0.25)), ("max_frames", dict(max_frames=float("inf")))):
        o = pkg.DurationsOpts(**kw)
        assert pkg.lib.xdtts_tacotron2_set_durations(None, C.byref(o)) == pkg.XDTTS_ERR_BAD_ARG
        assert field in pkg.lib.xdtts_last_error().decode(), (field, pkg.lib.xdtts_last_error())
    assert pkg.lib.xdtts_tacotron2_set_durations(None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert "handle" in pkg.lib.xdtts_last_error().decode()
    n = C.c_size_t()
    assert pkg.lib.xdtts_tacotron2_last_durations_count(None, C.byref(n)) == pkg.XDTTS_ERR_BAD_ARG
    a = np.ones((2, 4), dtype=np.float32)
    good = dict(cum_a=a, cum_b=a, nframes=[3, 4], n_valid=[2, 4])
    for what, kw in (("order", dict(order=[1, 1])), ("n_valid", dict(n_valid=[0, 4])), ("n_valid", dict(n_valid=[2, 5])),
                     ("nframes", dict(nframes=[-1, 4])), ("utt_of_chunk", dict(utt_of_chunk=[1, 1])), ("cum_b", dict(cum_b=None, batched=True))):
        for call in (lambda **k: pkg.durations_reference(**k), lambda **k: pkg.Tacotron2.durations_gather(_NullHandle(), **k)):
            with pytest.raises(pkg.XdttsError) as e:
                call(**{**good, **kw})
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and what in str(e.value), (what, str(e.value))
    # a good request on a null handle: the handle is what fails, after the arrays passed
    with pytest.raises(pkg.XdttsError) as e:
        pkg.Tacotron2.durations_gather(_NullHandle(), **good)
    assert "handle" in str(e.value)


class _NullHandle:
    _h = None


def _random_case(rng, B, T, batched, n_utt_chunks):
    cum_a = (rng.random((B, T)) * rng.choice([0.01, 1.0, 30.0], size=(B, 1))).astype(np.float32)
    cum_b = (rng.random((B, T)) * 5).astype(np.float32)
    nframes = rng.integers(0, 40, size=B).astype(np.int32)
    n_valid = rng.integers(1, T + 1, size=B).astype(np.int32)
    order = rng.permutation(B).astype(np.int32)
    utt, u = [], 0
    while len(utt) < B:
        utt += [u] * n_utt_chunks
        u += 1
    return dict(cum_a=cum_a, cum_b=cum_b, nframes=nframes, n_valid=n_valid, order=order, batched=batched, utt_of_chunk=utt[:B])


@pytest.mark.parametrize("B,T,batched,per_utt", [(1, 1, False, 1), (2, 7, True, 1), (6, 24, True, 3), (17, 24, True, 1), (33, 100, False, 4), (5, 512, True, 5)])
def test_numpy_restatement_equals_the_host_reference(pkg, B, T, batched, per_utt):
    """Row choice by parity, permutation, mask, multi-chunk bases, stats: random cases, bit for bit."""
    rng = np.random.default_rng(B * 1000 + T)
    case = _random_case(rng, B, T, batched, per_utt)
    case["cum_a"][0, 0] = np.float32(2.5 / 65536)  # a tie: to even
    o = pkg.DurationsOpts(on=1, min_frames=0.25, max_frames=20.0)
    assert_same(pkg.durations_reference(opts=o, **case), dr.durations(min_frames=0.25, max_frames=20.0, **case))
    # parity matters: flipping one slot's frame count by one changes its rows in batched mode only
    flipped = dict(case, nframes=case["nframes"].copy())
    flipped["nframes"][0] += 1
    same_rows = np.array_equal(pkg.durations_reference(**flipped)[0], pkg.durations_reference(**case)[0])
    assert same_rows == (not batched)


def test_64_bit_starts_at_16384_frame_chunks(pkg):
    B, T = 40, 3
    cum = np.tile(np.array([16000.0, 383.5, 0.5], dtype=np.float32), (B, 1))
    case = dict(cum_a=cum, cum_b=None, nframes=[16384] * B, n_valid=[3] * B, utt_of_chunk=[0] * B)
    got = pkg.durations_reference(**case)
    assert_same(got, dr.durations(**case))
    assert int(got[2][-1]) == (39 * 16384 + 16383) * 65536 + 32768 and int(got[2][-1]) > 2 ** 32
    assert got[3][0].n_frames == 40 * 16384 and got[3][0].sum_q16 == 40 * 16384 * 65536


def test_position_and_sample_maps(pkg):
    rng = np.random.default_rng(7)
    q = dr.q16(rng.random(9).astype(np.float32) * 6)
    st = np.concatenate([[0], np.cumsum(q.astype(np.uint64))[:-1]]).astype(np.uint64)
    F = int(np.ceil(q.astype(np.uint64).sum() / 65536)) + 1
    for x in (0.0, 1.0, 4.0, 8.0, 9.0, 0.5, 3.25, 8.999, 1e-9):
        assert pkg.durations_position(st, q, F, x) == dr.position(st, q, F, x), x
    assert pkg.durations_position(st, q, F, 0.0) == 0.0 and pkg.durations_position(st, q, 2, 9.0) == 1.0  # clamped
    for x in (-0.5, 9.5, float("nan")):
        assert np.isnan(pkg.durations_position(st, q, F, x))
    for s in (0, 65536, 12345678, 2 ** 40 + 17):
        for rate in (8000, 16000, 22050, 44100, 48000, 96000):
            assert pkg.durations_samples(s, 256, rate) == dr.samples(s, 256, rate), (s, rate)
    assert pkg.durations_samples(65536, 256, 7000) == -1


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_durations_plan_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "durations_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "durations_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "durations_plan.h"), encoding="utf-8").read()
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"resample_plan.h"}
    assert "hip/" not in src


# ---- discrimination ---------------------------------------------------------------------------------------------------------

def _oracle_case(orc64, blob, steps):
    B = len(steps)
    lens = dr.case_lens(B)
    cum = np.zeros((B, dr.WINDOW))
    prev = np.zeros((B, dr.WINDOW))
    for b in range(B):
        cum[b], prev[b] = dr.oracle_cum(orc64, blob, lens[b], b, steps[b])
    return lens, cum, prev


def test_every_plausible_mistake_moves_an_id_by_100_bounds(orc64, blob):
    """The 17-chunk batched case of the GPU test (the one with a sort and per-chunk parity), from the fp64 oracle: the right
    answer against the neighbour slot's row, the other parity buffer (the cumulative weights one step earlier), an unsorted
    order, unmasked padding, and a base off by one chunk (the 3-chunk utterance of the GPU test, in frames)."""
    name, _form, steps = [c for c in dr.ENGINE_CASES if c[0] == "batched-B17"][0]
    lens, cum, prev = _oracle_case(orc64, blob, steps)
    B = len(steps)
    order = sorted(range(B), key=lambda b: -steps[b])  # the batched engine's slots: longest first, stable
    right = [cum[b][:lens[b]] for b in range(B)]
    need = 100 * BOUND_CAP

    def differs(wrong):
        return max(float(np.abs(w - r).max()) for w, r in zip(wrong, right))

    slot_of = {c: j for j, c in enumerate(order)}
    neighbour = [cum[order[(slot_of[b] + 1) % B]][:lens[b]] for b in range(B)]
    other_parity = [prev[b][:lens[b]] for b in range(B)]
    unsorted = [cum[order[b]][:lens[b]] for b in range(B)]  # slot b taken for chunk b: it holds chunk order[b]
    assert differs(neighbour) >= need and differs(other_parity) >= need and differs(unsorted) >= need
    # each chunk alone, not just one of them, for the parity buffer: every chunk's last step moved some id
    assert min(float(np.abs(o - r).max()) for o, r in zip(other_parity, right)) >= need
    # unmasked padding: the layout shifts -- the id behind the first short chunk is read from the padding (weight 0) instead
    short = [b for b in range(B - 1) if lens[b] < dr.WINDOW][0]
    flat_right = np.concatenate(right)
    flat_unmasked = np.concatenate([cum[b] for b in range(B)])[:len(flat_right)]
    assert float(np.abs(flat_unmasked - flat_right).max()) >= need and cum[short][lens[short]:].max() == 0.0
    # a base off by one chunk, on the three-chunk utterance of the GPU test: the starts the stage would deliver with each later
    # chunk's base taken one chunk too far, or one chunk too short, against the right ones, in frames
    lens3, steps3 = list(dr.UTT3_LENS), list(dr.UTT3_STEPS)
    cum3 = np.zeros((3, dr.WINDOW), dtype=np.float32)
    for b in range(3):
        cum3[b] = dr.oracle_cum(orc64, blob, lens3[b], b, steps3[b])[0]
    right3 = dr.durations(cum3, None, steps3, lens3, utt_of_chunk=[0, 0, 0])[2].astype(np.int64)
    prefix = np.concatenate([[0], np.cumsum(steps3)])
    first = np.concatenate([[0], np.cumsum(lens3)])
    for shift in (+1, -1):
        wrong3 = right3.copy()
        for k in (1, 2):
            base = int(prefix[min(max(k + shift, 0), 3)])
            wrong3[first[k]:first[k + 1]] += (base - int(prefix[k])) * 65536
        for k in (1, 2):
            moved = np.abs(wrong3[first[k]:first[k + 1]] - right3[first[k]:first[k + 1]]).min() / 65536.0
            assert moved >= need, (shift, k, moved)


def test_id_anchored_contour_rejects_a_bad_pos_before_a_handle(pkg):
    """xdtts_synthesize_ids_contour_at_ids / _batch_contour_at_ids: pos is in ids, [0, n] and non-decreasing -- the message names
    the point (and the utterance), with null handles; a good contour gets as far as the null handles."""
    ids = np.arange(64, 74, dtype=np.int64)
    mel, audio, nf, ns = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_size_t(), C.c_size_t()

    def one(points):
        c = pkg.ProsodyContour(points)
        st = pkg.lib.xdtts_synthesize_ids_contour_at_ids(None, None, ids.ctypes.data, ids.size, None, 0, None, C.byref(c), C.byref(mel), C.byref(nf),
                                                         C.byref(audio), C.byref(ns))
        return st, pkg.lib.xdtts_last_error().decode()

    for points, word in (([(0, 1, 1, 1), (10.5, 1, 1.2, 1)], "point 1"), ([(-0.5, 1, 1, 1)], "point 0"), ([(float("nan"), 1, 1, 1)], "point 0"),
                         ([(4, 1, 1, 1), (3, 1, 1.2, 1)], "point 1"), ([(2, 1, 9.0, 1)], "pitch")):
        st, msg = one(points)
        assert st == pkg.XDTTS_ERR_BAD_ARG and word in msg, (points, msg)
    st, msg = one([(0, 1, 1, 1), (10, 1, 1.2, 1)])  # 10 = n: the end of the utterance
    assert st == pkg.XDTTS_ERR_BAD_ARG and "null" in msg, msg
    # the batch form names the utterance: utterance 1 has 4 ids
    lens = np.array([6, 4], dtype=np.int32)
    chunks = np.full((2, 6), 70, dtype=np.int64)
    uc = np.array([1, 1], dtype=np.int32)
    cs = pkg._contour_array([pkg.ProsodyContour([(6, 1, 1.1, 1)]), pkg.ProsodyContour([(5, 1, 1.1, 1)])], 2)
    mels, audios, nfs, nss = (C.POINTER(C.c_float) * 2)(), (C.POINTER(C.c_float) * 2)(), (C.c_size_t * 2)(), (C.c_size_t * 2)()
    st = pkg.lib.xdtts_synthesize_batch_contour_at_ids(None, None, chunks.ctypes.data, lens.ctypes.data, 2, 6, uc.ctypes.data, 2,
                                                       None, None, cs, mels, nfs, audios, nss)
    msg = pkg.lib.xdtts_last_error().decode()
    assert st == pkg.XDTTS_ERR_BAD_ARG and "utterance 1" in msg and "point 0" in msg, msg

