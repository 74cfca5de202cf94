"""The whole delivery chain at once (delivery.cpp: output rate -> compressor -> loudness target under a ceiling -> limiter), which
the tests of the single stages never switch on together: batch == single bit for bit, audio and stats, on both engines; every
stage off again == a handle that never had them; a level-0 join of either set of results is the same stream.

The mels have F = 2, 17, 18 and 40 frames = 256, 4096, 4352 and 9984 samples of the loop: below one compressor tile, exactly
one, just over one, several -- the smallest shapes at which a row offset or a launch extent of a record table can go wrong."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = (2, 17, 18, 40)
RATES = (8000, 48000)


def _mel(rng, F):
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32)


@pytest.fixture(scope="module")
def mels():
    rng = np.random.default_rng(20)
    return [_mel(rng, F) for F in FRAMES]


def _everything_on(pkg, v, rate):
    v.set_output_rate(rate)
    v.set_compressor(pkg.compressor_preset(1))  # drc
    v.set_loudness(-23.0, -1.0)
    v.set_limiter(5000)


def _everything_off(v):
    v.set_output_rate(22050)
    v.set_compressor(None)
    v.set_loudness(None, None)
    v.set_limiter(0)


def _fields(s):
    """every field of a stats struct, floats as their exact hex (the padding between fields is not part of the result)"""
    vals = [getattr(s, name) for name, _ in s._fields_]
    return tuple(x.hex() if isinstance(x, float) else x for x in vals)


def _stats(v):
    return [[_fields(s) for s in got] for got in (v.last_loudness(), v.last_limiter(), v.last_compressor())]


def _batch_equals_single(pkg, mels, rate):
    v = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        _everything_on(pkg, v, rate)
        single, loud, lim, comp = [], [], [], []
        for m, F in zip(mels, FRAMES):
            a = v.infer(m).copy()
            assert a.shape == (pkg.resample_plan(rate, 256 * (F - 1))["n_out"],) and np.all(np.isfinite(a)) and np.any(a != 0)
            single.append(a)
            s = _stats(v)
            assert [len(x) for x in s] == [1, 1, 1], (F, s)
            loud += s[0]
            lim += s[1]
            comp += s[2]
        got = [a.copy() for a in v.infer_batch(mels)]
        for a, b, F in zip(got, single, FRAMES):
            assert a.shape == b.shape and np.array_equal(a, b), (rate, F)
        assert _stats(v) == [loud, lim, comp]  # in the caller's order, whatever order the rows were laid out in
        # the stream stage sees the same utterances: a level-0 join of the singles == the same join of the batch's results
        gaps = [0, 100, 0, 37, 5]
        s1, off1 = v.join(single, gaps=gaps, rate=rate)
        s2, off2 = v.join(got, gaps=gaps, rate=rate)
        assert off1 == off2 and s1.dtype == s2.dtype and np.array_equal(s1, s2) and s1.size == sum(a.size for a in single) + sum(gaps)
    finally:
        v.close()


@pytest.mark.parametrize("rate", RATES)
def test_batch_equals_single_with_every_stage_on(pkg, mels, rate):
    _batch_equals_single(pkg, mels, rate)


@pytest.mark.parametrize("rate", RATES)
def test_batch_equals_single_on_the_launch_per_iteration_engine(pkg, mels, rate):
    os.environ["XDTTS_GL"] = "launch"
    try:
        _batch_equals_single(pkg, mels, rate)
    finally:
        del os.environ["XDTTS_GL"]


def test_every_stage_off_again_is_a_handle_that_never_had_them(pkg, mels):
    never = pkg.create_griffin_lim(iters=4, seed=5)
    was = pkg.create_griffin_lim(iters=4, seed=5)
    try:
        for rate in RATES:
            _everything_on(pkg, was, rate)
            on = [a.copy() for a in was.infer_batch(mels)]
            _everything_off(was)
            for m, a in zip(mels, on):
                b = never.infer(m)
                assert a.shape != b.shape and np.array_equal(was.infer(m), b)
                assert _stats(was) == [[], [], []]
            for a, b in zip(was.infer_batch(mels), never.infer_batch(mels)):
                assert np.array_equal(a, b)
            assert _stats(was) == [[], [], []]
    finally:
        never.close()
        was.close()
