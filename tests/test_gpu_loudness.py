"""The loudness stage on the device (loudness.hip; the definition: include/xdtts.h, restated in fp64 by tests/loudness_ref.py):
the measurement hook against fp64, ragged == single, off keeps every bit, the delivered level in the request paths (behind the
resampler, in the output normalisation's place) and the entry contracts."""
import functools
import os

import numpy as np
import pytest

import loudness_ref as lr
from conftest import synth_ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=8, seed=3)
    yield v
    v.close()


@functools.lru_cache(maxsize=None)
def _case(Q, N):
    """(input, fp64 measurement) of one hook case: computed once, shared, never written to."""
    x = lr.speech_like(Q, N)
    x.setflags(write=False)
    return x, lr.measure(x, Q)


def _mel(rng, F):
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32)


def _check_against_ref(pkg, got, x, m, taps64, where):
    """One struct against the restatement; returns (mean-square error / tolerance, true-peak error / bound)."""
    assert (got.blocks, got.gated_blocks) == (m["blocks"], m["gated_blocks"]), where
    assert got.gain == 1.0, where
    if m["mean_square"] == 0.0:
        assert got.mean_square == 0.0 and got.lufs == -np.inf, where
        r_ms = 0.0
    else:
        # n eps kappa <= 5e5 2^-53 200 = 1.1e-8 (tests/test_loudness_cpu.py asserts kappa), times ten for the block means.  With
        # equal counts a different SET of gated blocks would move Z by far more: the same blocks are gated.
        r_ms = abs(got.mean_square - m["mean_square"]) / m["mean_square"] / 1e-7
        assert r_ms <= 1.0, (where, r_ms)
        assert abs(got.lufs - m["lufs"]) <= 1e-6, where
    assert got.sample_peak == float(np.max(np.abs(x))), where  # exact
    tp, _, bound = lr.true_peak(x, taps64)
    r_tp = abs(got.true_peak - tp) / bound if bound > 0 else 0.0
    assert got.true_peak >= got.sample_peak and r_tp <= 1.0, (where, r_tp)
    return r_ms, r_tp


@pytest.mark.parametrize("Q", lr.GPU_RATES)
def test_hook_against_fp64(pkg, voc, Q):
    """blocks and gated_blocks equal; mean_square within 1e-7 relative; the true peak within (24 + 2) 2^-24 sum |t| |x| of the
    fp64 evaluation with the library's own taps; the sample peak exact.  Lengths: no block, exactly one, a segment across a
    sub-block boundary, more than 64 segments, more than one group.  MI355X, worst ratios (mean square to its 1e-7 / true peak
    to its bound): 0.0000 / 0.038 (8000), 0.0000 / 0.000 (11025), 0.0000 / 0.024 (22050), 0.0001 / 0.017 (48000), 0.0009 / 0.011
    (96000) -- profiles/loudness.txt."""
    taps64 = pkg.true_peak_filter().astype(np.float64)
    worst_ms = worst_tp = 0.0
    for N in lr.lengths(Q):
        x, m = _case(Q, N)
        got = voc.loudness(x, Q)
        r_ms, r_tp = _check_against_ref(pkg, got, x, m, taps64, (Q, N))
        worst_ms, worst_tp = max(worst_ms, r_ms), max(worst_tp, r_tp)
    print("loudness hook rate %d: worst mean-square error / 1e-7 = %.4f, worst true-peak error / bound = %.4f" % (Q, worst_ms, worst_tp))
    assert voc.last_timings()["mel_to_linear_ms"] > 0.0  # ms[0]: the stage alone
    assert voc.last_loudness() == [] and np.isnan(voc.get_loudness()[0])  # the hook is no delivering call; no target is set


def test_hook_on_the_anchors(voc):
    """The device reads the analytic anchors as the restatement does: the 997 Hz sine at 48 kHz, the fs/4 burst at 0 dBTP."""
    got = voc.loudness(lr.sine(48000).astype(np.float32), 48000)
    assert got.lufs == pytest.approx(-3.010, abs=0.001) and got.gated_blocks == got.blocks == 27
    got = voc.loudness(lr.quarter_rate_burst().astype(np.float32), 48000)
    assert 20 * np.log10(got.true_peak) == pytest.approx(0.0, abs=0.01) and 20 * np.log10(got.sample_peak) == pytest.approx(-3.01, abs=0.01)


@pytest.mark.parametrize("Q", (8000, 48000))
def test_ragged_equals_single(pkg, voc, Q):
    xs = [_case(Q, N)[0] for N in lr.ragged_lengths(Q)]
    single = [voc.loudness(x, Q).astuple() for x in xs]
    for order in (list(range(5)), list(range(5))[::-1]):
        got = voc.loudness_batch([xs[u] for u in order], Q)
        for k, u in enumerate(order):
            assert np.array_equal(np.array(got[k].astuple()), np.array(single[u])), (Q, order, u)


def test_off_keeps_every_bit(pkg, model):
    """A handle that had a target set and then cleared returns the bits of a handle that never had one: infer, infer_batch,
    synthesize_sequence.  The setting round-trips; a bad value leaves it alone."""
    rng = np.random.default_rng(2)
    mels = [_mel(rng, F) for F in (37, 9, 120)]
    ids = [synth_ids(n, seed=40 + i) for i, n in enumerate([24, 31])]
    o = pkg.default_opts(fixed_frames_per_id=1.5, dropout_seed=2)
    never = pkg.create_griffin_lim(iters=8, seed=3)
    setv = pkg.create_griffin_lim(iters=8, seed=3)
    try:
        assert all(np.isnan(v) for v in setv.get_loudness())
        setv.set_loudness(-16.0, -1.0)
        assert setv.get_loudness() == (-16.0, -1.0)
        for t, c in ((0.5, None), (-71.0, None), (-16.0, 6.5), (-16.0, -21.0), (float("inf"), None)):
            with pytest.raises(pkg.XdttsError) as e:
                setv.set_loudness(t, c)
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and setv.get_loudness() == (-16.0, -1.0)
        on = setv.infer(mels[0])
        assert len(setv.last_loudness()) == 1 and not np.array_equal(on, never.infer(mels[0]))
        setv.set_loudness(None, None)
        assert all(np.isnan(v) for v in setv.get_loudness())
        for m in mels:
            assert np.array_equal(setv.infer(m), never.infer(m))
            assert setv.last_loudness() == []
        for a, b in zip(setv.infer_batch(mels), never.infer_batch(mels)):
            assert np.array_equal(a, b)
        (_, a1), (_, a2) = pkg.synthesize_sequence(model, setv, ids, None, opts=o), pkg.synthesize_sequence(model, never, ids, None, opts=o)
        for a, b in zip(a1, a2):
            assert a.size > 0 and np.array_equal(a, b)
        assert setv.last_loudness() == []
    finally:
        never.close()
        setv.close()


@pytest.mark.parametrize("Q", (22050, 8000, 48000))
def test_delivered_level(pkg, Q):
    """With a target the delivered signal is gain x raw (raw: the same call with the target off and output_normalise 0), the gain
    is the restatement's on raw, and the restatement reads the delivered signal at the target.  F = 7 (the launch-per-iteration
    engine) is shorter than one block at every rate: unscaled, L = -inf.  F = 40 and 120: the persistent engine."""
    v = pkg.create_griffin_lim(iters=8, seed=4)
    rng = np.random.default_rng(0)
    v.set_output_rate(Q)
    v.set_opts(output_normalise=3)  # (the default: with a target on it is not applied)
    try:
        for F in (7, 40, 120):
            mel = _mel(rng, F)
            v.set_loudness(None, None)
            v.set_opts(output_normalise=0)
            raw = v.infer(mel).copy()
            v.set_opts(output_normalise=3)
            n_out = pkg.resample_plan(Q, 256 * (F - 1))["n_out"]
            m = lr.measure(raw, Q)
            assert raw.shape == (n_out,) and m["blocks"] == pkg.loudness_plan(Q, n_out)["n_blocks"]
            for target in (-16.0, -23.0):
                v.set_loudness(target, None)
                got = v.infer(mel)
                (l,) = v.last_loudness()
                assert got.shape == (n_out,)
                assert (l.blocks, l.gated_blocks) == (m["blocks"], m["gated_blocks"]), (F, target)
                if F == 7:  # too short for one block
                    assert m["blocks"] == 0 and l.gain == 1.0 and l.lufs == -np.inf and np.array_equal(got, raw)
                    continue
                want = lr.gain(m["mean_square"], m["true_peak"], target)
                assert abs(l.gain - want) <= 1e-6 * want, (F, target)
                assert np.abs(got.astype(np.float64) - l.gain * raw.astype(np.float64)).max() <= 4e-7 * float(np.abs(got).max()), (F, target)
                assert abs(lr.measure(got, Q)["lufs"] - target) <= 1e-4, (F, target)
            # a target the ceiling stops: 0 LUFS would need peaks far past 0.1
            C = -20.0
            v.set_loudness(0.0, C)
            got = v.infer(mel)
            (l,) = v.last_loudness()
            if F == 7:
                assert l.gain == 1.0 and np.array_equal(got, raw)
                continue
            assert lr.gain(m["mean_square"], m["true_peak"], 0.0) * m["true_peak"] > 10 ** (C / 20)
            assert abs(l.gain * l.true_peak - 10 ** (C / 20)) <= 2e-7, F
            assert np.abs(got.astype(np.float64) - l.gain * raw.astype(np.float64)).max() <= 4e-7 * float(np.abs(got).max()), F
            assert lr.measure(got, Q)["lufs"] < 0.0, F
            # ... and the delivered samples peak there: within the device's own fp32 true-peak error and the rounding of the scaling
            tp_d, _, bound = lr.true_peak(got, pkg.true_peak_filter().astype(np.float64))
            assert abs(tp_d - 10 ** (C / 20)) <= bound + 2.0 ** -23 * 10 ** (C / 20), F
    finally:
        v.close()


def test_entry_contracts_at_16000(pkg, model):
    """batch_shape 4, Q = 16000, target -16 LUFS under -1 dBTP: infer_batch == infer, infer_batch(prosody=) == infer_prosody,
    synthesize_sequence == a loop of synthesize, bit for bit, samples and structs; last_loudness in the caller's order."""
    Q = 16000
    v = pkg.create_griffin_lim(iters=8, seed=3)
    v.set_opts(batch_shape=4)
    v.set_output_rate(Q)
    v.set_loudness(-16.0, -1.0)
    try:
        rng = np.random.default_rng(11)
        Fs = (37, 9, 120, 64)
        mels = [_mel(rng, F) for F in Fs]
        single, structs = [], []
        for mel in mels:
            single.append(v.infer(mel).copy())
            structs.append(v.last_loudness()[0].astuple())
        assert structs[1][4] == 0 and structs[1][3] == 1.0 and structs[2][5] > 0 and structs[2][3] != 1.0  # F = 9: no block
        got = v.infer_batch(mels)
        ll = v.last_loudness()
        assert len(ll) == 4
        for a, b, l, s in zip(got, single, ll, structs):
            assert np.array_equal(a, b) and l.astuple() == s
        # the caller's order, whatever order the launches take the utterances in
        got = v.infer_batch(mels[::-1])
        for a, b, l, s in zip(got, single[::-1], v.last_loudness(), structs[::-1]):
            assert np.array_equal(a, b) and l.astuple() == s
        pros = [pkg.Prosody(rate=1.25), pkg.Prosody(), pkg.Prosody(rate=0.8, pitch=1.1), pkg.Prosody(pitch=0.9)]
        single, structs = [], []
        for mel, p in zip(mels, pros):
            single.append(v.infer_prosody(mel, p).copy())
            structs.append(v.last_loudness()[0].astuple())
        got = v.infer_batch(mels, prosody=pros)
        for a, b, l, s in zip(got, single, v.last_loudness(), structs):
            assert np.array_equal(a, b) and l.astuple() == s
        ids = [synth_ids(n, seed=70 + i) for i, n in enumerate([24, 31, 18])]
        o = pkg.default_opts(fixed_frames_per_id=1.5, dropout_seed=2)
        want, structs = [], []
        for x in ids:
            want.append(pkg.synthesize(model, v, x, opts=o))
            structs.append(v.last_loudness()[0].astuple())
        seq_mels, seq_audios = pkg.synthesize_sequence(model, v, ids, None, opts=o)
        ll = v.last_loudness()
        assert len(ll) == 3
        for (m1, a1), m2, a2, l, s in zip(want, seq_mels, seq_audios, ll, structs):
            assert np.array_equal(m1, m2) and np.array_equal(a1, a2) and l.astuple() == s
    finally:
        v.close()


def test_a_demoted_handles_retry_delivers_the_same_rule(pkg, capfd):
    """A persistent launch whose exchange times out (test hooks: a short spin budget and a slow workgroup) demotes the handle;
    the run is repeated on the launch-per-iteration engine, the loudness stage included: gain x that engine's audio."""
    Q = 16000
    v = pkg.create_griffin_lim(iters=8, seed=6)
    mel = _mel(np.random.default_rng(9), 80)
    v.set_output_rate(Q)
    v.set_loudness(-23.0, -1.0)
    os.environ["XDTTS_GL_SPINS"] = "50"
    os.environ["XDTTS_GL_SLOW"] = "2"
    try:
        b = v.infer(mel)
    finally:
        del os.environ["XDTTS_GL_SPINS"], os.environ["XDTTS_GL_SLOW"]
    assert "persistent Griffin-Lim exchange timed out" in capfd.readouterr().err
    (l,) = v.last_loudness()
    v.set_loudness(None, None)
    v.set_opts(output_normalise=0)
    a = v.infer(mel)  # (the demoted handle: the launch-per-iteration engine)
    m = lr.measure(a, Q)
    want = lr.gain(m["mean_square"], m["true_peak"], -23.0, -1.0)
    assert b.shape == a.shape and m["gated_blocks"] > 0 and abs(l.gain - want) <= 1e-6 * want
    assert np.abs(b.astype(np.float64) - l.gain * a.astype(np.float64)).max() <= 4e-7 * float(np.abs(b).max())
    v.close()
