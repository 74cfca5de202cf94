"""The dynamic range compressor on the device (compressor.hip; the definition: include/xdtts.h, evaluated sample by sample in the
serial form on the host by xdtts_compressor_reference, which tests/test_compressor_cpu.py holds against the fp64 restatement):
the hook against the reference bit for bit, ragged == single, and the stage's place in the handle's delivery chain."""
import functools

import numpy as np
import pytest

import compressor_ref as cr
import loudness_ref as lr
from conftest import synth_ids

pytestmark = pytest.mark.gpu

TILE = cr.TILE


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=4, seed=3)
    yield v
    v.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _mel(rng, F):
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32)


def _floor(N, seed, amp=1e-4):
    return (amp * np.random.Generator(np.random.PCG64(seed)).standard_normal(N)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _hook_cases():
    """(name, rate, settings, input): computed once, shared, never written to"""
    out = []
    for n in (1, 2, 255, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
        out.append(("n=%d" % n, 22050, cr.DRC, cr.signal("impulses", 22050, n)))
    x = _floor(3 * TILE, 1)
    x[TILE - 1], x[2 * TILE] = 0.9, -0.7   # the last sample of a tile, the first of another: carries in both directions
    out.append(("bursts at tile edges", 22050, cr.DRC, x))
    x = _floor(5 * TILE, 2)
    x[100] = 1.0
    out.append(("release tail over the tiles", 8000, dict(cr.DRC, release_ms=2000.0), x))
    x = _floor(4 * TILE, 3)
    x[4 * TILE - 100] = -1.0
    out.append(("attack ramp over the tiles", 96000, dict(cr.DRC, attack_ms=100.0), x))
    x = np.zeros(4 * TILE + 77, dtype=np.float32)
    x[TILE - 300:TILE - 1] = 0.5 * np.sin(0.3 * np.arange(299))
    x[3 * TILE + 1:3 * TILE + 200] = 0.3
    out.append(("zeros down to the floor", 8000, dict(cr.DRC, attack_ms=0.1, release_ms=1.0), x))
    out.append(("ratio 20, hard knee", 22050, dict(cr.DRC, ratio=20.0, knee_db=0.0), cr.signal("speech", 22050, 2 * TILE + 9)))
    out.append(("ratio 1.5, knee 24", 22050, dict(cr.DRC, ratio=1.5, knee_db=24.0), cr.signal("speech", 22050, 2 * TILE + 9)))
    out.append(("makeup only", 22050, dict(cr.DEFAULT, makeup_db=6.0), cr.signal("steps", 22050, TILE + 33)))
    for c in out:
        c[3].setflags(write=False)
    return tuple(out)


@pytest.mark.parametrize("k", range(14))
def test_hook_equals_the_reference(pkg, voc, k):
    """xdtts_griffinlim_compress == xdtts_compressor_reference, samples and stats, bit for bit."""
    name, Q, c, x = _hook_cases()[k]
    comp = pkg.Compressor(**c)
    want, wst = pkg.compressor_reference(x, Q, comp)
    got, st = voc.compress(x, Q, comp)
    assert np.array_equal(_bits(got), _bits(want)), name
    assert st.astuple() == wst.astuple() and st.engaged == 1 and st.peak == np.abs(x).max(), name
    if c["ratio"] > 1.0:
        assert st.compressed > 0 and st.max_over == -pkg.compressor_plan(Q, comp)["T"], name
        assert not np.array_equal(got, x), name
    else:
        assert st.compressed == 0 and np.array_equal(_bits(got), _bits(x * np.float32(10.0 ** (6.0 / 20.0)))), name
    if name.startswith("zeros"):
        assert pkg.compressor_envelope(x, Q, comp)[2 * TILE] == cr.L_FLOOR   # the stretch reaches the floor
    assert voc.last_compressor() == [] and voc.get_compressor() is None   # the hook is no delivering call; nothing is set


def test_hook_identity_and_silence(pkg, voc):
    x = cr.signal("impulses", 22050, TILE + 5)
    got, st = voc.compress(x, 22050, pkg.Compressor())
    assert np.array_equal(_bits(got), _bits(x)) and st.astuple() == (0.0, 0, 0, 0)
    z = np.zeros(TILE + 5, dtype=np.float32)
    z[7] = -0.0
    got, st = voc.compress(z, 22050, pkg.compressor_preset(1))
    assert np.array_equal(_bits(got), _bits(z)) and st.astuple() == (0.0, 0, 0, 0)
    assert st.astuple() == pkg.compressor_reference(z, 22050, pkg.compressor_preset(1))[1].astuple()


def test_ragged_equals_single(pkg, voc):
    comp = pkg.compressor_preset(1)
    xs = [cr.signal("speech", 22050, n, seed=i) for i, n in enumerate((1, TILE, TILE + 1, 9000, 3))]
    xs[3] = np.zeros(9000, dtype=np.float32)   # one utterance of the batch is not engaged
    single = [voc.compress(x, 22050, comp) for x in xs]
    assert single[3][1].engaged == 0 and single[2][1].engaged == 1
    for order in (list(range(5)), list(range(5))[::-1]):
        outs, stats = voc.compress_batch([xs[u] for u in order], 22050, comp)
        for k, u in enumerate(order):
            assert np.array_equal(_bits(outs[k]), _bits(single[u][0])) and stats[k].astuple() == single[u][1].astuple(), (order, u)
    xs[3] = cr.signal("speech", 22050, 9000, seed=3)
    single = [voc.compress(x, 22050, comp) for x in xs]
    for order in (list(range(5)), list(range(5))[::-1]):
        outs, stats = voc.compress_batch([xs[u] for u in order], 22050, comp)
        for k, u in enumerate(order):
            assert np.array_equal(_bits(outs[k]), _bits(single[u][0])) and stats[k].astuple() == single[u][1].astuple(), (order, u)
            assert stats[k].astuple() == pkg.compressor_reference(xs[u], 22050, comp)[1].astuple()


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))


@pytest.mark.parametrize("Q", (22050, 8000))
def test_infer_is_compress_of_infer(pkg, Q):
    """output_normalise none: infer with the compressor on == compress(infer with it off), bit for bit, stats included; with rms
    normalisation the delivered rms is the target; None and the identity restore the bits of a handle that never had it."""
    comp = pkg.compressor_preset(1)
    v = pkg.create_griffin_lim(iters=4, seed=5)
    never = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        mel = _mel(np.random.default_rng(4), 8)
        for h in (v, never):
            h.set_output_rate(Q)
            h.set_opts(output_normalise=0)
        raw = never.infer(mel).copy()
        assert v.get_compressor() is None
        v.set_compressor(comp)
        assert v.get_compressor().astuple() == comp.astuple()
        got = v.infer(mel).copy()
        (st,) = v.last_compressor()
        want, wst = never.compress(raw, Q, comp)
        assert np.array_equal(_bits(got), _bits(want)) and st.astuple() == wst.astuple() and st.engaged == 1 and st.compressed > 0
        assert not np.array_equal(got, raw)
        # rms normalisation behind the stage: the level rule holds for what is delivered
        for h in (v, never):
            h.set_opts(output_normalise=2, rms_target=0.1)
        got = v.infer(mel).copy()
        assert abs(_rms(got) - 0.1) <= 1e-6
        assert not np.array_equal(got, never.infer(mel))
        # off, and the identity: the bits of the handle that never had it
        for setting in (None, pkg.Compressor()):
            v.set_compressor(setting)
            assert np.array_equal(_bits(v.infer(mel)), _bits(never.infer(mel))) and v.last_compressor() == []
        assert v.get_compressor().astuple() == pkg.Compressor().astuple()
        with pytest.raises(pkg.XdttsError) as e:
            v.set_compressor(pkg.Compressor(ratio=0.5))
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and "ratio" in str(e.value) and v.get_compressor().astuple() == pkg.Compressor().astuple()
    finally:
        v.close()
        never.close()


def test_loudness_target_holds_behind_the_compressor(pkg):
    T = -20.0
    comp = pkg.compressor_preset(1)
    v = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        mel = _mel(np.random.default_rng(6), 60)
        v.set_opts(output_normalise=0)
        raw = v.infer(mel).copy()
        squeezed, _ = v.compress(raw, 22050, comp)
        v.set_compressor(comp)
        v.set_loudness(T, None)
        got = v.infer(mel).copy()
        (l,) = v.last_loudness()
        (st,) = v.last_compressor()
        assert st.engaged == 1 and st.compressed > 0
        assert l.astuple()[:3] == v.loudness(squeezed, 22050).astuple()[:3]   # the measurement saw the compressed signal
        assert abs(l.lufs + 20.0 * np.log10(l.gain) - T) <= 1e-6
        assert abs(lr.measure(got, 22050)["lufs"] - T) <= 1e-4
        # ... and under the limiter
        v.set_loudness(-10.0, -3.0)
        v.set_limiter(2000)
        got = v.infer(mel).copy()
        (l,), (ls,), (st2,) = v.last_loudness(), v.last_limiter(), v.last_compressor()
        assert st2.astuple() == st.astuple()
        want, wls = pkg.limiter_reference(squeezed, 22050, l.gain, 10.0 ** (-3.0 / 20.0), 2000)
        assert np.array_equal(_bits(got), _bits(want)) and ls.astuple() == wls.astuple()
    finally:
        v.close()


def test_sequence_and_batch(pkg, model):
    """The two pieces of a sequence equal the single calls; the batch equals the single calls and last_compressor follows the
    caller's order; the document's pieces carry the stage."""
    comp = pkg.compressor_preset(1)
    o = pkg.default_opts(fixed_frames_per_id=1.5, dropout_seed=2)
    ids = [synth_ids(n, seed=70 + i) for i, n in enumerate([24, 31])]
    v = pkg.create_griffin_lim(iters=4, seed=3)
    try:
        v.set_compressor(comp)
        single, stats = [], []
        for u in ids:
            _m, a = pkg.synthesize(model, v, u, opts=o)
            single.append(a.copy())
            stats.append(v.last_compressor()[0].astuple())
        _m, seq = pkg.synthesize_sequence(model, v, ids, None, opts=o, want_mels=False)
        ls = v.last_compressor()
        assert len(ls) == 2
        for k in range(2):
            assert np.array_equal(_bits(seq[k]), _bits(single[k])) and ls[k].astuple() == stats[k]
        # the batch at the single-utterance shape, in two orders
        v.set_opts(batch_shape=4)
        rng = np.random.default_rng(11)
        mels = [_mel(rng, F) for F in (20, 9, 37)]
        one, st1 = [], []
        for m in mels:
            one.append(v.infer(m).copy())
            st1.append(v.last_compressor()[0].astuple())
        assert len(set(st1)) == 3
        for order in ((0, 1, 2), (2, 0, 1)):
            got = v.infer_batch([mels[u] for u in order])
            ls = v.last_compressor()
            assert len(ls) == 3
            for k, u in enumerate(order):
                assert np.array_equal(_bits(got[k]), _bits(one[u])) and ls[k].astuple() == st1[u], (order, u)
        # a document at level 0, fp32: its pieces are the single calls' audio
        so = pkg.StreamOpts(format=0, dither=0, level=0, fade=0)
        _m, stream, off = pkg.synthesize_document(model, v, ids, (0, 100, 0), so, opts=o, want_mels=False)
        for k in range(2):
            assert np.array_equal(_bits(stream[off[k]:off[k] + single[k].size]), _bits(single[k]))
        assert [s.astuple() for s in v.last_compressor()] == stats
    finally:
        v.close()


def test_entry_contracts(pkg, voc):
    x = np.zeros(100, dtype=np.float32)
    ok = pkg.compressor_preset(1)
    for kw in (dict(ratio=0.99), dict(ratio=21.0), dict(threshold_db=1.0), dict(knee_db=float("nan")), dict(attack_ms=0.05), dict(release_ms=2001.0),
               dict(makeup_db=-1.0)):
        bad = pkg.Compressor(**dict(cr.DRC, **kw))
        for f in (lambda: voc.compress(x, 22050, bad), lambda: voc.compress_batch([x, x], 22050, bad), lambda: pkg.compressor_reference(x, 22050, bad)):
            with pytest.raises(pkg.XdttsError) as e:
                f()
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and list(kw)[0] in str(e.value), kw
    for f in (lambda: voc.compress(x, 7999, ok), lambda: voc.compress(x, 96001, ok), lambda: voc.compress(x[:0], 22050, ok),
              lambda: voc.compress_batch([], 22050, ok)):
        with pytest.raises(pkg.XdttsError) as e:
            f()
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
