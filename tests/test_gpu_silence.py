"""The silence stage on the device (csrc/silence.hip), bit for bit -- every decision of the definition is an integer or a
comparison and a fade is one fp32 multiply, so no tolerance appears anywhere: the stage alone against xdtts_silence_reference on
the crafted signals of tests/silence_ref.py (among them more windows than k_sil_plan's workgroup has lanes, and windows that
straddle every tile boundary); the ragged batch against the single call in two orders; the stage through the chain -- infer on
both engines, every other stage on at 48000, infer_batch, the sequence, synthesize -- against the reference applied to what the
same call delivers with the stage off; a document against stream_ref's join of the trimmed pieces; and off == never set."""
import functools
import os

import numpy as np
import pytest

import silence_ref as sr
import stream_ref
from conftest import synth_ids

pytestmark = pytest.mark.gpu

CASES = sr.cases()
CASE_IDS = [c[0] for c in CASES]
FRAMES = (2, 17, 18, 40)
# The mel's quiet edges: 8 and 12 frames at ln(1e-5) beside frames of uniform(-7, -1) -- through mel -> linear (x^(1/1.7) of a
# non-negative combination) their magnitudes lie about 43 dB under the loud frames', 70 and 115 ms long behind the analysis window
EDGES = dict(threshold_db=-20.0, min_sound_ms=0.0, lead_ms=20.0, trail_ms=40.0)
HARSH = dict(threshold_db=-6.0, min_sound_ms=10.0, lead_ms=10.0, trail_ms=15.0, max_pause_ms=40.0)   # as many cuts as a setting gives
BREAK = 6615                                                                        # 300 ms at 22050


def _sil(pkg, s):
    return pkg.Silence(**s)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _fields(st):
    return tuple(x.hex() if isinstance(x, float) else x for x in st.astuple())


@pytest.fixture(scope="module")
def voc(pkg):
    v = pkg.create_griffin_lim(iters=4, seed=5)
    yield v
    v.close()


@functools.lru_cache(maxsize=None)
def _mels():
    """FRAMES frames each; the 40-frame one has its first 8 and last 12 frames at the log floor ln(1e-5)"""
    rng = np.random.default_rng(20)
    out = [(rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32) for F in FRAMES]
    out[3][:, :8] = np.float32(np.log(1e-5))
    out[3][:, -12:] = np.float32(np.log(1e-5))
    return out


def _ids():
    return [synth_ids(n, seed=70 + i) for i, n in enumerate([40, 33, 52])]


# ---- the stage alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_stage_alone_equals_the_reference(pkg, voc, case):
    name, Q, s, x = CASES[case]
    want, wst = pkg.silence_reference(x, Q, _sil(pkg, s))
    got, st = voc.trim(x, Q, _sil(pkg, s))
    assert _fields(st) == _fields(wst), (name, st.astuple(), wst.astuple())
    assert got.size == st.n_out and _same(got, want), name


@pytest.mark.parametrize("order", ((0, 1, 2, 3, 4, 5, 6), (2, 6, 0, 4, 1, 5, 3)))
def test_ragged_batch_equals_the_single_call(pkg, voc, order):
    """seven utterances under one setting, the all-zero one, the one-sample one and the 1200-window one among them"""
    by = {c[0]: c[3] for c in CASES}
    s = _sil(pkg, sr.settings(threshold_db=-30.0, max_pause_ms=100.0))
    xs = [by["zeros"], by["n=1"], by["1200 windows"], by["clicks"], by["pauses even noise"], by["all sound"], by["n=4097"]]
    xs = [xs[i] for i in order]
    outs, stats = voc.trim_batch(xs, 22050, s)
    for u, x in enumerate(xs):
        one, st1 = voc.trim(x, 22050, s)
        ref, rst = pkg.silence_reference(x, 22050, s)
        assert _fields(stats[u]) == _fields(st1) == _fields(rst), (order, u)
        assert _same(outs[u], one) and _same(one, ref), (order, u)


# ---- through the chain -----------------------------------------------------------------------------------------------------

def _everything_on(pkg, v, rate):
    v.set_output_rate(rate)
    v.set_compressor(pkg.compressor_preset(1))
    v.set_loudness(-23.0, -1.0)
    v.set_limiter(5000)


def _infer_on_and_off(pkg, rate, everything):
    v = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        if everything:
            _everything_on(pkg, v, rate)
        s = _sil(pkg, sr.settings(**EDGES))
        m = _mels()[3]
        y = v.infer(m).copy()
        assert v.last_silence() == [] and v.get_silence() is None
        v.set_silence(s)
        assert v.get_silence().astuple() == s.astuple()
        z = v.infer(m).copy()
        want, wst = pkg.silence_reference(y, rate, s)
        got = v.last_silence()
        assert len(got) == 1 and _fields(got[0]) == _fields(wst)
        assert z.size == wst.n_out and _same(z, want)            # n_samples == n_out
        assert wst.any_sound == 1 and wst.n_in == y.size
        if not everything:   # (the compressor lifts the edges towards the threshold: there the bits alone are held)
            assert wst.lead_cut > 0 and wst.trail_cut > 0
        if everything:
            assert [len(x) for x in (v.last_loudness(), v.last_limiter(), v.last_compressor())] == [1, 1, 1]
        # the batch and its stats, in the caller's order
        v.set_silence(None)
        ys = [a.copy() for a in v.infer_batch(_mels())]
        v.set_silence(s)
        zs = [a.copy() for a in v.infer_batch(_mels())]
        got = v.last_silence()
        assert len(got) == len(ys)
        for u, (a, b) in enumerate(zip(ys, zs)):
            want, wst = pkg.silence_reference(a, rate, s)
            assert _fields(got[u]) == _fields(wst) and b.size == wst.n_out and _same(b, want), (rate, u)
        assert _same(zs[3], z)
    finally:
        v.close()


def test_infer_and_infer_batch_deliver_the_trimmed_utterance(pkg):
    _infer_on_and_off(pkg, 22050, False)


def test_with_every_other_stage_on_at_48000(pkg):
    _infer_on_and_off(pkg, 48000, True)


@pytest.mark.parametrize("everything", (False, True))
def test_on_the_launch_per_iteration_engine(pkg, everything):
    os.environ["XDTTS_GL"] = "launch"
    try:
        _infer_on_and_off(pkg, 48000 if everything else 22050, everything)
    finally:
        del os.environ["XDTTS_GL"]


@pytest.fixture(scope="module")
def seq(pkg, model, voc):
    """the sequence with the stage off: computed once"""
    o = pkg.default_opts(fixed_frames_per_id=2.0, dropout_seed=2)
    _m, audios = pkg.synthesize_sequence(model, voc, _ids(), None, opts=o, want_mels=False)
    return o, [a.copy() for a in audios]


def test_sequence_and_synthesize(pkg, model, voc, seq):
    o, ys = seq
    s = _sil(pkg, sr.settings(**HARSH))
    refs = [pkg.silence_reference(y, 22050, s) for y in ys]
    voc.set_silence(s)
    try:
        _m, zs = pkg.synthesize_sequence(model, voc, _ids(), None, opts=o, want_mels=False)
        zs = [a.copy() for a in zs]
        got = voc.last_silence()
        _m, one = pkg.synthesize(model, voc, _ids()[1], opts=o)
        one, got_one = one.copy(), voc.last_silence()
    finally:
        voc.set_silence(None)
    assert len(got) == 3 and len(got_one) == 1
    for u, (z, (want, wst)) in enumerate(zip(zs, refs)):
        assert _fields(got[u]) == _fields(wst) and z.size == wst.n_out and _same(z, want), u
    assert _fields(got_one[0]) == _fields(refs[1][1]) and _same(one, refs[1][0])


# ---- document --------------------------------------------------------------------------------------------------------------

def _zero_runs(stream, off, pieces, gaps):
    for u in range(len(pieces) - 1):
        a, b = off[u] + pieces[u].size, off[u + 1]
        assert b - a == gaps[u + 1] >= BREAK and not stream[a:b].any(), u


def test_document_joins_the_trimmed_pieces(pkg, model, voc, seq):
    """three utterances with a 300 ms break: the stream is stream_ref's join of the three trimmed pieces, at level 0 (with the
    document's own edge fade beside the stage's) and at programme level (the pieces enter unlevelled, one gain for the stream)"""
    o, ys = seq
    gaps = (0, BREAK, BREAK, 0)
    s = _sil(pkg, sr.settings(**HARSH))
    pieces = [pkg.silence_reference(y, 22050, s)[0] for y in ys]
    raw_voc = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        raw_voc.set_opts(output_normalise=0)
        _m, raw = pkg.synthesize_sequence(model, raw_voc, _ids(), None, opts=o, want_mels=False)
        raw_pieces = [pkg.silence_reference(a.copy(), 22050, s)[0] for a in raw]
    finally:
        raw_voc.close()
    voc.set_silence(s)
    try:
        _m, stream, off = pkg.synthesize_document(model, voc, _ids(), gaps, pkg.StreamOpts(format=0, fade=30), opts=o, want_mels=False)
        stats0 = voc.last_silence()
        voc.set_loudness(-20.0, -1.0)
        _m, pcm, off1 = pkg.synthesize_document(model, voc, _ids(), gaps, pkg.StreamOpts(format=1, level=1), opts=o, want_mels=False)
        ls = voc.last_loudness()
    finally:
        voc.set_loudness(None)
        voc.set_silence(None)
    want, woff = stream_ref.join(pieces, gaps, stream_ref.F32_FMT, fade=30)
    assert off == woff and stream.size == want.size == sum(p.size for p in pieces) + 2 * BREAK
    assert _same(stream, want)
    assert [st.n_out for st in stats0] == [p.size for p in pieces]
    _zero_runs(stream, off, pieces, gaps)
    stream0, woff1 = stream_ref.join(raw_pieces, gaps, stream_ref.F32_FMT)
    assert off1 == woff1 and len(ls) == 1
    wl = voc.loudness(stream0, 22050)
    assert ls[0].mean_square == wl.mean_square and ls[0].true_peak == wl.true_peak
    assert np.array_equal(pcm, stream_ref.encode(stream0 * np.float32(ls[0].gain), stream_ref.PCM16))
    _zero_runs(pcm, off1, raw_pieces, gaps)


# ---- off is off ------------------------------------------------------------------------------------------------------------

def test_set_then_cleared_is_a_handle_that_never_had_the_stage(pkg, model, seq):
    o, ys = seq
    gaps = (0, 441, 0, 100)
    never = pkg.create_griffin_lim(iters=4, seed=5)
    was = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        was.set_silence(_sil(pkg, sr.settings(**HARSH)))
        assert was.infer(_mels()[3]).size < never.infer(_mels()[3]).size
        was.set_silence(None)
        assert was.get_silence() is None
        assert _same(was.infer(_mels()[3]), never.infer(_mels()[3])) and was.last_silence() == []
        for a, b in zip(was.infer_batch(_mels()), never.infer_batch(_mels())):
            assert _same(a, b)
        assert was.last_silence() == []
        _m, a, offa = pkg.synthesize_document(model, was, _ids(), gaps, pkg.StreamOpts(format=1), opts=o, want_mels=False)
        _m, b, offb = pkg.synthesize_document(model, never, _ids(), gaps, pkg.StreamOpts(format=1), opts=o, want_mels=False)
        assert offa == offb and np.array_equal(a, b) and was.last_silence() == []
        # ... and the bits of the sequence the module's handle computed before the stage was ever set on it
        want, _ = stream_ref.join(ys, gaps, stream_ref.PCM16)
        assert np.array_equal(a, want)
    finally:
        never.close()
        was.close()
