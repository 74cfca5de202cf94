"""The whole magnitude chain at once (magnitude.cpp: tracker and pitch target -> contour -> handle timbre -> SPSI initial phase),
which the tests of the single stages never switch on together: batch == single bit for bit, audio and F0 stats, on both engines;
one synthesize == the vocoder entry on the mel it returns; everything off again == a handle that never had it.

The mels have F = 2, 24, 25 and 40 frames: the shortest request, exactly one SPSI segment, one segment and a frame (the chained
form), and two segments -- the smallest shapes at which a row offset of a record table can go wrong.  Every contour has a rate
other than 1, so no utterance keeps its frame count."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = (2, 24, 25, 40)
RATES = (0.5, 2.0, 1.25, 0.8)
TIMBRE = dict(vtl=1.12, breath=0.25, seed=9)


def _mel(rng, F):
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32)


@pytest.fixture(scope="module")
def mels():
    rng = np.random.default_rng(20)
    return [_mel(rng, F) for F in FRAMES]


def _contours(pkg):
    """a pitch ramp, a gain dip and a rate that is never 1"""
    return [pkg.ProsodyContour([(0.0, r, 0.9, 1.0), (0.5, r, 1.1, 0.7), (1.0, r, 1.25, 1.2)]) for r in RATES]


def _targets(pkg):
    return [pkg.PitchTarget(hz=180.0), pkg.PitchTarget(factor=1.1, range=0.5), pkg.PitchTarget(hz=110.0, range=1.5), pkg.PitchTarget(factor=0.9)]


def _everything_on(pkg, v):
    v.set_timbre(pkg.Timbre(**TIMBRE))
    v.set_phase_init(1)


def _fields(s):
    vals = [getattr(s, name) for name, _ in s._fields_]
    return tuple(x.hex() if isinstance(x, float) else x for x in vals)


def _batch_equals_single(pkg, mels):
    v = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        _everything_on(pkg, v)
        cons, tgts = _contours(pkg), _targets(pkg)
        single, f0 = [], []
        for m, c, t, F in zip(mels, cons, tgts, FRAMES):
            a = v.infer_pitch_target(m, t, c).copy()
            assert a.shape == (256 * (pkg.prosody_contour_frames(c, F) - 1),) and np.all(np.isfinite(a)) and np.any(a != 0)
            assert a.shape != (256 * (F - 1),)
            single.append(a)
            s = v.last_f0()
            assert len(s) == 1 and s[0].n_frames == F
            f0.append(_fields(s[0]))
        got = [a.copy() for a in v.infer_batch_pitch_target(mels, tgts, cons)]
        for a, b, F in zip(got, single, FRAMES):
            assert a.shape == b.shape and np.array_equal(a, b), F
        assert [_fields(s) for s in v.last_f0()] == f0  # in the caller's order
    finally:
        v.close()


def test_batch_equals_single_with_the_whole_chain_on(pkg, mels):
    _batch_equals_single(pkg, mels)


def test_batch_equals_single_on_the_launch_per_iteration_engine(pkg, mels):
    os.environ["XDTTS_GL"] = "launch"
    try:
        _batch_equals_single(pkg, mels)
    finally:
        del os.environ["XDTTS_GL"]


def test_synthesize_equals_the_vocoder_entry_on_the_mel_it_returns(pkg):
    golden = np.load(os.path.join(ROOT, "tests", "golden", "tacotron2_small.npz"))
    model = pkg.Tacotron2.synthetic(seed=int(golden["weight_seed"]))
    v = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        _everything_on(pkg, v)
        c, t = _contours(pkg)[0], _targets(pkg)[0]
        o = pkg.default_opts(fixed_frames_per_id=2.0, dropout_seed=2)
        mel, audio = pkg.synthesize(model, v, golden["ids"].astype(np.int64), opts=o, contour=c, target=t)
        audio, f0 = audio.copy(), [_fields(s) for s in v.last_f0()]
        assert len(f0) == 1 and audio.shape == (256 * (pkg.prosody_contour_frames(c, mel.shape[1]) - 1),)
        again = v.infer_pitch_target(mel, t, c)
        assert np.array_equal(audio, again) and [_fields(s) for s in v.last_f0()] == f0
    finally:
        v.close()
        model.close()


def test_everything_off_again_is_a_handle_that_never_had_it(pkg, mels):
    never = pkg.create_griffin_lim(iters=4, seed=5)
    was = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        _everything_on(pkg, was)
        on = [a.copy() for a in was.infer_batch_pitch_target(mels, _targets(pkg), _contours(pkg))]
        assert len(was.last_f0()) == len(mels)
        was.set_timbre(None)
        was.set_phase_init(0)
        for m, a in zip(mels, on):
            b = never.infer(m)
            assert a.shape != b.shape and np.array_equal(was.infer(m), b)
            assert was.last_f0() == []
        for a, b in zip(was.infer_batch(mels), never.infer_batch(mels)):
            assert np.array_equal(a, b)
        assert was.last_f0() == []
    finally:
        never.close()
        was.close()
