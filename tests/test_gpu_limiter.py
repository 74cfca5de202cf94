"""The look-ahead true-peak limiter on the device (limiter.hip; the definition: include/xdtts.h, evaluated sample by sample on
the host by xdtts_limiter_reference, which tests/test_limiter_cpu.py holds against the fp64 restatement): the hook against the
reference bit for bit, ragged == single, off keeps every bit, on but not binding, the delivered level in the request paths, the
batch, the document at programme level and the entry contracts."""
import functools

import numpy as np
import pytest

import limiter_ref as lm
import loudness_ref as lr
import stream_ref as sr
from conftest import synth_ids

pytestmark = pytest.mark.gpu

T_LUFS, C_DBTP = -10.0, -3.0
C_LIN = 10.0 ** (C_DBTP / 20.0)


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=8, seed=3)
    yield v
    v.close()


@functools.lru_cache(maxsize=None)
def _case(Q, us, N):
    """one hook input: computed once, shared, never written to"""
    x = lm.signal(Q, us, N)
    x.setflags(write=False)
    return x


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _mel(rng, F):
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32)


@pytest.mark.parametrize("us", lm.LOOKAHEADS)
@pytest.mark.parametrize("Q", lm.GPU_RATES)
def test_hook_equals_the_reference(pkg, voc, Q, us):
    """xdtts_griffinlim_limit == xdtts_limiter_reference, samples and stats, bit for bit: lengths 1, H, 2 H + 1, TILE - 1, TILE,
    TILE + 1, 2 TILE + 2 H + 5 of the feature signal (impulses at both ends and across the tile boundary, peaks 2 H - 1 and 4 H + 2
    apart, a plateau, the quarter-rate burst), and the case where no sample needs limiting: fl(x G)."""
    p = pkg.limiter_plan(Q, us)
    assert p == {"half_width": lm.half_width(Q, us), "tile": lm.TILE}
    for N in lm.lengths(Q, us):
        x = _case(Q, us, N)
        want, wst = pkg.limiter_reference(x, Q, lm.GAIN0, lm.CEIL, us)
        got, st = voc.limit(x, Q, lm.GAIN0, lm.CEIL, us)
        assert np.array_equal(_bits(got), _bits(want)), (Q, us, N)
        assert st.astuple() == wst.astuple() and st.engaged == 1 and st.half_width == p["half_width"] and st.limited > 0, (Q, us, N)
    x = _case(Q, us, lm.lengths(Q, us)[-1])
    got, st = voc.limit(x, Q, 0.5, 1.0, us)
    assert np.array_equal(_bits(got), _bits(x * np.float32(0.5))) and st.astuple() == (1.0, p["half_width"], 1, 0)
    assert np.array_equal(_bits(got), _bits(pkg.limiter_reference(x, Q, 0.5, 1.0, us)[0]))
    assert voc.last_timings()["mel_to_linear_ms"] > 0.0  # ms[0]: the stage alone
    assert voc.last_limiter() == [] and voc.get_limiter() == 0  # the hook is no delivering call; nothing is set


@pytest.mark.parametrize("Q,us", [(22050, 5000), (96000, 10000)])
def test_ragged_equals_single(pkg, voc, Q, us):
    L = lm.lengths(Q, us)
    xs = [_case(Q, us, N) for N in (L[0], L[6], L[1], L[5], L[4])]
    single = [voc.limit(x, Q, lm.GAIN0, lm.CEIL, us) for x in xs]
    for order in (list(range(5)), list(range(5))[::-1]):
        outs, stats = voc.limit_batch([xs[u] for u in order], Q, lm.GAIN0, lm.CEIL, us)
        for k, u in enumerate(order):
            assert np.array_equal(_bits(outs[k]), _bits(single[u][0])) and stats[k].astuple() == single[u][1].astuple(), (Q, order, u)


def _ids():
    return [synth_ids(n, seed=70 + i) for i, n in enumerate([24, 31])]


GAPS = (0, 441, 100)


def test_off_keeps_every_bit(pkg, model):
    """A handle that had the limiter set and then cleared returns the bits of a handle that never had it: infer, infer_batch,
    synthesize_sequence, synthesize_document at level 0 and at level 1 (both handles with the same target and ceiling).  The
    setting round-trips; a bad value leaves it alone."""
    rng = np.random.default_rng(2)
    mels = [_mel(rng, F) for F in (37, 9, 120)]
    o = pkg.default_opts(fixed_frames_per_id=1.5, dropout_seed=2)
    never = pkg.create_griffin_lim(iters=8, seed=3)
    setv = pkg.create_griffin_lim(iters=8, seed=3)
    try:
        for v in (never, setv):
            v.set_loudness(T_LUFS, C_DBTP)
        assert setv.get_limiter() == 0
        setv.set_limiter(5000)
        assert setv.get_limiter() == 5000
        for bad in (499, 10001, -1, 1 << 20):
            with pytest.raises(pkg.XdttsError) as e:
                setv.set_limiter(bad)
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and setv.get_limiter() == 5000
        on = setv.infer(mels[2])
        assert len(setv.last_limiter()) == 1 and setv.last_limiter()[0].engaged == 1
        assert not np.array_equal(on, never.infer(mels[2]))
        setv.set_limiter(0)
        assert setv.get_limiter() == 0
        for m in mels:
            assert np.array_equal(setv.infer(m), never.infer(m))
            assert setv.last_limiter() == [] and setv.last_loudness()[0].astuple() == never.last_loudness()[0].astuple()
        for a, b in zip(setv.infer_batch(mels), never.infer_batch(mels)):
            assert np.array_equal(a, b)
        assert setv.last_limiter() == []
        (_, a1), (_, a2) = pkg.synthesize_sequence(model, setv, _ids(), None, opts=o), pkg.synthesize_sequence(model, never, _ids(), None, opts=o)
        for a, b in zip(a1, a2):
            assert a.size > 0 and np.array_equal(a, b)
        for level in (0, 1):
            so = pkg.StreamOpts(format=1, dither=1, dither_seed=5, level=level, fade=32)
            _m, s1, _ = pkg.synthesize_document(model, setv, _ids(), GAPS, so, opts=o, want_mels=False)
            _m, s2, _ = pkg.synthesize_document(model, never, _ids(), GAPS, so, opts=o, want_mels=False)
            assert s1.size > 0 and np.array_equal(s1, s2), level
            assert setv.last_limiter() == []
    finally:
        never.close()
        setv.close()


def test_on_but_not_binding(pkg):
    """A target, a ceiling and the limiter set, but a ceiling that does not bind: the bits of the limiter off; engaged is 0."""
    v = pkg.create_griffin_lim(iters=8, seed=4)
    rng = np.random.default_rng(1)
    try:
        v.set_loudness(-40.0, 6.0)
        for F in (40, 120):
            mel = _mel(rng, F)
            v.set_limiter(0)
            off = v.infer(mel).copy()
            loff = v.last_loudness()[0].astuple()
            assert loff[3] * loff[1] < 10.0 ** (6.0 / 20.0) and loff[3] != 1.0  # the ceiling does not bind; something was scaled
            v.set_limiter(1500)
            on = v.infer(mel)
            (st,) = v.last_limiter()
            assert np.array_equal(_bits(on), _bits(off)) and v.last_loudness()[0].astuple() == loff
            assert st.astuple() == (1.0, pkg.limiter_plan(22050, 1500)["half_width"], 0, 0)
        # no ceiling at all: the limiter has nothing to keep, nothing new is launched
        v.set_loudness(-40.0, None)
        v.set_limiter(0)
        off = v.infer(mel).copy()
        v.set_limiter(1500)
        assert np.array_equal(_bits(v.infer(mel)), _bits(off)) and v.last_limiter() == []
    finally:
        v.close()


@pytest.mark.parametrize("Q", (22050, 8000, 48000))
def test_delivered_level(pkg, Q):
    """-10 LUFS under -3 dBTP with a 5 ms look-ahead.  On the raw run (target off, output_normalise 0) the ceiling binds:
    g0 TP > c.  The delivered signal is xdtts_limiter_reference of raw with the returned gain, bit for bit, stats included; the
    gain is the restatement's uncapped g0; the delivered loudness (fp64) is higher than the one-gain delivery's.  F = 7: no block,
    unscaled, engaged 0."""
    us = 5000
    v = pkg.create_griffin_lim(iters=8, seed=4)
    rng = np.random.default_rng(0)
    v.set_output_rate(Q)
    try:
        for F in (7, 40, 120):
            mel = _mel(rng, F)
            v.set_loudness(None, None)
            v.set_limiter(0)
            v.set_opts(output_normalise=0)
            raw = v.infer(mel).copy()
            v.set_opts(output_normalise=3)
            m = lr.measure(raw, Q)
            v.set_loudness(T_LUFS, C_DBTP)
            one_gain = v.infer(mel).copy()
            v.set_limiter(us)
            got = v.infer(mel)
            (l,) = v.last_loudness()
            (st,) = v.last_limiter()
            if F == 7:
                assert m["blocks"] == 0 and l.gain == 1.0 and np.array_equal(_bits(got), _bits(raw))
                assert st.astuple() == (1.0, pkg.limiter_plan(Q, us)["half_width"], 0, 0)
                continue
            g0 = lr.gain(m["mean_square"], m["true_peak"], T_LUFS)  # no ceiling
            assert g0 * m["true_peak"] > C_LIN, (F, g0 * m["true_peak"])  # the precondition: the ceiling binds
            assert abs(l.gain - g0) <= 1e-6 * g0, F
            want, wst = pkg.limiter_reference(raw, Q, l.gain, C_LIN, us)
            assert np.array_equal(_bits(got), _bits(want)), (Q, F)
            assert st.astuple() == wst.astuple() and st.engaged == 1 and st.limited > 0 and st.min_gain < 1.0, (Q, F)
            assert lr.measure(got, Q)["lufs"] > lr.measure(one_gain, Q)["lufs"], (Q, F)
    finally:
        v.close()


def test_batch_equals_single(pkg):
    """infer_batch with ragged F: every utterance equals its single call, samples and both structs, in the caller's order."""
    Q = 16000
    v = pkg.create_griffin_lim(iters=8, seed=3)
    v.set_opts(batch_shape=4)
    v.set_output_rate(Q)
    v.set_loudness(T_LUFS, C_DBTP)
    v.set_limiter(2000)
    try:
        rng = np.random.default_rng(11)
        mels = [_mel(rng, F) for F in (37, 9, 120, 64)]
        single, loud, lim = [], [], []
        for mel in mels:
            single.append(v.infer(mel).copy())
            loud.append(v.last_loudness()[0].astuple())
            lim.append(v.last_limiter()[0].astuple())
        assert lim[1][2] == 0 and lim[2][2] == 1 and lim[2][3] > 0  # F = 9: no block, not engaged
        for order in ((0, 1, 2, 3), (3, 2, 1, 0)):
            got = v.infer_batch([mels[u] for u in order])
            ll, ls = v.last_loudness(), v.last_limiter()
            assert len(ll) == 4 and len(ls) == 4
            for k, u in enumerate(order):
                assert np.array_equal(_bits(got[k]), _bits(single[u])) and ll[k].astuple() == loud[u] and ls[k].astuple() == lim[u], (order, u)
    finally:
        v.close()


@pytest.mark.parametrize("fmt,dither", [(sr.PCM16, 1), (sr.ULAW, 0)])
def test_stream_at_programme_level(pkg, voc, fmt, dither):
    """Level 1 with the limiter: the bytes are stream_ref's encode of the reference limiter applied to the formed fp32 stream
    (fades and gaps in it) with the measurement's uncapped gain; gap bytes are the exact zeros, also under dither; one loudness
    struct and one stats struct come back."""
    Q, us, fade = 22050, 5000, 64
    N = int(1.5 * Q)
    x = lr.speech_like(Q, N)
    cuts = [0, N // 3 + 7, 2 * N // 3 - 5, N]
    audios = [np.ascontiguousarray(x[a:b]) for a, b in zip(cuts, cuts[1:])]
    g = int(0.3 * Q)
    gaps = [5, g, g, 3]
    stream0, off = sr.join(audios, gaps, 0, fade=fade)
    m = lr.measure(stream0, Q)
    g0 = lr.gain(m["mean_square"], m["true_peak"], T_LUFS)
    assert g0 * m["true_peak"] > C_LIN
    try:
        voc.set_loudness(T_LUFS, C_DBTP)
        voc.set_limiter(us)
        got, goff = voc.join(audios, gaps, rate=Q, opts=pkg.StreamOpts(format=fmt, dither=dither, dither_seed=9, level=1, fade=fade))
        ls, st = voc.last_loudness(), voc.last_limiter()
    finally:
        voc.set_limiter(0)
        voc.set_loudness(None)
    assert len(ls) == 1 and len(st) == 1 and list(goff) == list(off)
    assert abs(ls[0].gain - g0) <= 1e-6 * g0
    limited, wst = pkg.limiter_reference(stream0, Q, ls[0].gain, C_LIN, us)
    assert st[0].astuple() == wst.astuple() and st[0].engaged == 1 and st[0].limited > 0
    want = np.full(stream0.size, sr.SILENCE[fmt], dtype=sr.DTYPE[fmt])
    for a, o in zip(audios, off):
        want[o:o + a.size] = sr.encode(limited[o:o + a.size], fmt, dither, 9, np.arange(o, o + a.size))
    assert np.array_equal(_bits(got), _bits(want))
    inside = np.zeros(stream0.size, dtype=bool)
    for a, o in zip(audios, off):
        inside[o:o + a.size] = True
    assert np.all(np.asarray(got)[~inside] == sr.SILENCE[fmt]) and (~inside).sum() == sum(gaps)


def test_document_at_programme_level(pkg, model):
    """xdtts_synthesize_document at level 1 with the limiter: the utterances enter unlevelled, the stream is limited once."""
    o = pkg.default_opts(fixed_frames_per_id=2.0, dropout_seed=2)
    us = 5000
    v = pkg.create_griffin_lim(iters=8, seed=3)
    try:
        v.set_opts(output_normalise=0)
        _m, raw = pkg.synthesize_sequence(model, v, _ids(), None, opts=o, want_mels=False)
        raw = [a.copy() for a in raw]
        v.set_opts(output_normalise=3)
        stream0, off = sr.join(raw, GAPS, 0, fade=32)
        m = lr.measure(stream0, 22050)
        assert lr.gain(m["mean_square"], m["true_peak"], T_LUFS) * m["true_peak"] > C_LIN
        v.set_loudness(T_LUFS, C_DBTP)
        v.set_limiter(us)
        so = pkg.StreamOpts(format=1, dither=1, dither_seed=3, level=1, fade=32)
        _m, pcm, goff = pkg.synthesize_document(model, v, _ids(), GAPS, so, opts=o, want_mels=False)
        ls, st = v.last_loudness(), v.last_limiter()
    finally:
        v.close()
    assert len(ls) == 1 and len(st) == 1 and st[0].engaged == 1 and list(goff) == list(off)
    limited, wst = pkg.limiter_reference(stream0, 22050, ls[0].gain, C_LIN, us)
    assert st[0].astuple() == wst.astuple()
    want = np.zeros(stream0.size, dtype=sr.DTYPE[sr.PCM16])
    for a, k in zip(raw, off):
        want[k:k + a.size] = sr.encode(limited[k:k + a.size], sr.PCM16, 1, 3, np.arange(k, k + a.size))
    assert np.array_equal(pcm, want)


def test_entry_contracts(pkg, voc):
    x = np.zeros(100, dtype=np.float32)
    bad = [dict(us=499), dict(us=10001), dict(us=0), dict(us=-3), dict(rate=7999), dict(rate=96001), dict(c=0.0), dict(c=-1.0),
           dict(c=float("nan")), dict(g=float("inf")), dict(x=np.zeros(0, dtype=np.float32))]
    voc.set_limiter(1500)
    try:
        for kw in bad:
            a = dict(x=x, rate=22050, g=1.0, c=0.5, us=5000)
            a.update(kw)
            for f in (lambda: voc.limit(a["x"], a["rate"], a["g"], a["c"], a["us"]),
                      lambda: voc.limit_batch([x, a["x"]], a["rate"], a["g"], a["c"], a["us"]),
                      lambda: pkg.limiter_reference(a["x"], a["rate"], a["g"], a["c"], a["us"])):
                with pytest.raises(pkg.XdttsError) as e:
                    f()
                assert e.value.status == pkg.XDTTS_ERR_BAD_ARG, kw
            assert voc.get_limiter() == 1500
        with pytest.raises(pkg.XdttsError) as e:
            voc.limit_batch([], 22050, 1.0, 0.5, 5000)
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    finally:
        voc.set_limiter(0)
