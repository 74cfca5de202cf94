"""The output-rate stage on the device (resample.hip: k_resample; the definition: include/xdtts.h, restated in fp64 by
tests/resample_ref.py): the parity hook against fp64 with the library's own taps as the filter, ragged == single, the identity,
the stage's place in the request paths (behind the loop, in front of the output normalisation) and the entry contracts."""
import os

import numpy as np
import pytest

import resample_ref as rr
from conftest import synth_ids

pytestmark = pytest.mark.gpu

HOOK_RATES = (8000, 11025, 44100, 48000, 32000)  # L 160 / M 441 (the longest window), 1 / 2, 2 / 1, 320 / 147, L = 640
HOOK_N = (1, 2, 255, 256, 257, 885, 4097, 9216)


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=8, seed=3)
    yield v
    v.close()


@pytest.fixture(scope="module")
def taps(pkg):
    """The library's own fp32 taps per rate, as the fp64 filter of the reference: kernel parity does not depend on libm."""
    return {Q: pkg.resample_filter(Q).astype(np.float64) for Q in HOOK_RATES}


def _rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)))


def _mel(rng, F):
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32)


def _edge(Q):
    """Output samples next to either end that the zero extension reaches: H / M of them (H / L input samples); the larger of the two counts is taken."""
    p = rr.plan(Q)
    return max(p["half_len"] // p["L"], p["half_len"] // p["M"]) + 1


@pytest.mark.parametrize("Q", HOOK_RATES)
def test_hook_against_fp64(pkg, voc, taps, Q):
    """|y - y_f64| <= (c[m] + 2) 2^-24 a[m] per sample, for uniform noise and for the all-ones vector (which away from the
    ends returns 1 within the same bound).  MI355X, worst ratio to the bound: 0.21 (8000), 0.28 (11025), 0.19 (44100), 0.20
    (48000), 0.15 (32000) -- profiles/resample.txt."""
    rng = np.random.Generator(np.random.PCG64(1000 + Q))
    worst = 0.0
    for N in HOOK_N:
        for kind in ("uniform", "ones"):
            x = rng.uniform(-1.0, 1.0, N).astype(np.float32) if kind == "uniform" else np.ones(N, np.float32)
            y = voc.resample(x, Q)
            ref, c, a = rr.convolve(x, taps[Q], Q)
            assert y.dtype == np.float32 and y.shape == ref.shape == (pkg.resample_plan(Q, N)["n_out"],), (Q, N)
            bound = rr.bound(c, a)
            assert np.all(a > 0)  # (every output meets at least the tap at or next to it)
            ratio = float(np.max(np.abs(y.astype(np.float64) - ref) / bound))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (Q, N, kind, ratio)
            e = _edge(Q)
            if kind == "ones" and y.size > 2 * e:
                mid = slice(e, y.size - e)
                assert np.all(np.abs(y[mid].astype(np.float64) - 1.0) <= bound[mid]), (Q, N)
    print("resample hook rate %d: worst |y - y_f64| / bound = %.4f" % (Q, worst))


def test_ragged_equals_single(voc):
    rng = np.random.Generator(np.random.PCG64(7))
    lengths = (1, 4097, 2, 885, 256)
    xs = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in lengths]
    for Q in (8000, 48000, 32000):
        single = [voc.resample(x, Q).copy() for x in xs]
        for order in (list(range(5)), list(range(5))[::-1]):
            got = voc.resample_batch([xs[u] for u in order], Q)
            for k, u in enumerate(order):
                assert got[k].shape == single[u].shape and np.array_equal(got[k], single[u]), (Q, order, u)
    # the hook takes its rate as an argument, whatever the handle's option; 22050 copies
    assert voc.get_output_rate() == 22050
    assert np.array_equal(voc.resample(xs[3], 22050), xs[3])
    voc.resample(xs[1], 8000)
    assert voc.last_timings()["mel_to_linear_ms"] > 0.0  # ms[0]: the stage alone


def test_tail_of_an_input_whose_index_products_pass_2_32(pkg, voc):
    """Q = 8008 (L = 572, M = 1575): m M passes 2^32 at m = 2 726 982.  The last outputs of a 7.6 M-sample input against fp64."""
    Q, N = 8008, 7_600_000
    p = pkg.resample_plan(Q, N)
    assert (p["L"], p["M"]) == (572, 1575) and (p["n_out"] - 1) * p["M"] > 2 ** 32
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.uniform(-1.0, 1.0, N).astype(np.float32)
    y = voc.resample(x, Q)
    h = pkg.resample_filter(Q).astype(np.float64)
    first = -(-(2 ** 32) // p["M"])
    for m in (np.arange(first - 600, first + 600), np.arange(p["n_out"] - 1200, p["n_out"])):  # across the 2^32 line, and the tail
        ref, c, a = rr.convolve(x, h, Q, m=m)
        assert np.all(np.abs(y[m].astype(np.float64) - ref) <= rr.bound(c, a))
        assert _rms(ref) > 0.3


def test_identity_keeps_every_bit(pkg, voc, model):
    """Rate 22050 set explicitly: infer, infer_batch and synthesize_sequence return the bits of a handle that never had the
    option set; the option round-trips."""
    rng = np.random.default_rng(2)
    mels = [_mel(rng, F) for F in (37, 9, 120)]
    ids = [synth_ids(n, seed=40 + i) for i, n in enumerate([24, 31])]
    o = pkg.default_opts(fixed_frames_per_id=1.5, dropout_seed=2)
    never = pkg.create_griffin_lim(iters=8, seed=3)
    setv = pkg.create_griffin_lim(iters=8, seed=3)
    try:
        assert setv.get_output_rate() == 22050
        setv.set_output_rate(16000)
        assert setv.get_output_rate() == 16000
        for bad in (7999, 96001, 22051, 0, -1):
            with pytest.raises(pkg.XdttsError) as e:
                setv.set_output_rate(bad)
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and setv.get_output_rate() == 16000
        setv.set_output_rate(22050)
        assert setv.get_output_rate() == 22050
        for m in mels:
            assert np.array_equal(setv.infer(m), never.infer(m))
        for a, b in zip(setv.infer_batch(mels), never.infer_batch(mels)):
            assert np.array_equal(a, b)
        (_, a1), (_, a2) = pkg.synthesize_sequence(model, setv, ids, None, opts=o), pkg.synthesize_sequence(model, never, ids, None, opts=o)
        for a, b in zip(a1, a2):
            assert a.size > 0 and np.array_equal(a, b)
    finally:
        never.close()
        setv.close()


def _composition(pkg, v, F=37):
    """output_normalise 0: infer at rate Q == the hook on infer at 22050, bit for bit -- the same kernel on the same bits."""
    mel = _mel(np.random.default_rng(9), F)
    v.set_opts(output_normalise=0)
    v.set_output_rate(22050)
    a = v.infer(mel).copy()
    assert a.shape == (256 * (F - 1),)
    for Q in (8000, 16000, 48000):
        v.set_output_rate(Q)
        b = v.infer(mel)
        assert b.shape == (pkg.resample_plan(Q, a.size)["n_out"],), Q
        assert np.array_equal(b, v.resample(a, Q)), Q
        # infer_linear is the loop alone: it stays at 22050
        assert v.infer_linear(v.mel_to_linear(mel)).shape == a.shape
    v.set_output_rate(22050)
    assert np.array_equal(v.infer(mel), a)
    return a


def test_composition_on_the_persistent_engine(pkg):
    v = pkg.create_griffin_lim(iters=8, seed=6)
    try:
        _composition(pkg, v)
    finally:
        v.close()


def test_composition_on_the_launch_per_iteration_engine(pkg):
    v = pkg.create_griffin_lim(iters=8, seed=6)
    os.environ["XDTTS_GL"] = "launch"
    try:
        _composition(pkg, v)
    finally:
        del os.environ["XDTTS_GL"]
        v.close()


def test_a_demoted_handles_retry_goes_through_the_stage_again(pkg, capfd):
    """A persistent launch whose exchange times out (test hooks: a short spin budget and a slow workgroup) demotes the handle;
    the run is repeated on the launch-per-iteration engine, the stage included: N' samples, the hook's bits on that engine's
    audio."""
    v = pkg.create_griffin_lim(iters=8, seed=6)
    mel = _mel(np.random.default_rng(9), 80)
    v.set_opts(output_normalise=0)
    v.set_output_rate(16000)
    os.environ["XDTTS_GL_SPINS"] = "50"
    os.environ["XDTTS_GL_SLOW"] = "2"
    try:
        b = v.infer(mel)
    finally:
        del os.environ["XDTTS_GL_SPINS"], os.environ["XDTTS_GL_SLOW"]
    assert "persistent Griffin-Lim exchange timed out" in capfd.readouterr().err
    v.set_output_rate(22050)
    a = v.infer(mel)  # (the demoted handle: the launch-per-iteration engine)
    assert b.shape == (pkg.resample_plan(16000, a.size)["n_out"],) and np.array_equal(b, v.resample(a, 16000))
    v.close()


@pytest.mark.parametrize("Q", (8000, 48000))
def test_normalisation_follows_the_resampler(pkg, Q):
    """Peak 1, rms = target, target capped by the peak -- for the signal the caller receives, with the tolerances
    tests/test_gpu_output_normalise.py uses for the same statements at 22050."""
    v = pkg.create_griffin_lim(iters=8, seed=4)
    rng = np.random.default_rng(0)
    v.set_output_rate(Q)
    for F in (7, 40):  # the launch-per-iteration engine (F < 16) and the persistent one
        mel = _mel(rng, F)
        v.set_opts(output_normalise=0)
        raw = v.infer(mel).astype(np.float64)
        n_out = pkg.resample_plan(Q, 256 * (F - 1))["n_out"]
        assert raw.shape == (n_out,) and _rms(raw) > 0
        for mode, target in ((1, 0.1), (2, 0.1), (2, 0.25), (3, 0.1), (3, 0.6)):
            v.set_opts(output_normalise=mode, rms_target=target)
            got = v.infer(mel)
            assert got.shape == (n_out,)
            scale = float(np.dot(got.astype(np.float64), raw) / np.dot(raw, raw))  # the delivered signal is the resampled one, scaled
            assert np.abs(got - scale * raw).max() <= 4e-7 * float(np.abs(got).max()), (F, mode)
            if mode == 2 or (mode == 3 and target == 0.1):
                assert abs(_rms(got) - target) <= 2e-7 * target / 0.1 + 1e-7
            elif mode == 3:  # rms 0.6 would push the peaks past 1: the scale stops at 1 / max|y|
                assert abs(float(np.abs(got).max()) - 1.0) <= 2e-7 and _rms(got) < target and target / _rms(raw) * np.abs(raw).max() > 1.0
            else:
                assert float(np.abs(got).max()) == 1.0
    v.close()


def test_entry_contracts_at_16000(pkg, model):
    """batch_shape 4, Q = 16000: infer_batch == infer, infer_batch(prosody=) == infer_prosody, synthesize_sequence == a loop of
    synthesize, bit for bit; n_samples = resample_plan(hop (F' - 1)) in each."""
    Q = 16000
    v = pkg.create_griffin_lim(iters=8, seed=3)
    v.set_opts(batch_shape=4)
    v.set_output_rate(Q)
    n_out = lambda n: pkg.resample_plan(Q, n)["n_out"]
    try:
        rng = np.random.default_rng(11)
        Fs = (37, 9, 120, 64)
        mels = [_mel(rng, F) for F in Fs]
        single = [v.infer(m).copy() for m in mels]
        for a, b, F in zip(v.infer_batch(mels), single, Fs):
            assert b.shape == (n_out(256 * (F - 1)),) and np.array_equal(a, b), F
        pros = [pkg.Prosody(rate=1.25), pkg.Prosody(), pkg.Prosody(rate=0.8, pitch=1.1), pkg.Prosody(pitch=0.9)]
        single = [v.infer_prosody(m, p).copy() for m, p in zip(mels, pros)]
        for a, b, F, p in zip(v.infer_batch(mels, prosody=pros), single, Fs, pros):
            assert b.shape == (n_out(256 * (pkg.prosody_frames(F, p.rate) - 1)),) and np.array_equal(a, b), F
        ids = [synth_ids(n, seed=70 + i) for i, n in enumerate([24, 31, 18])]
        o = pkg.default_opts(fixed_frames_per_id=1.5, dropout_seed=2)
        want = [pkg.synthesize(model, v, x, opts=o) for x in ids]
        seq_mels, seq_audios = pkg.synthesize_sequence(model, v, ids, None, opts=o)
        for (m1, a1), m2, a2 in zip(want, seq_mels, seq_audios):
            assert np.array_equal(m1, m2)
            assert a1.shape == (n_out(256 * (m1.shape[1] - 1)),) and np.array_equal(a1, a2)
        # the batch pipeline delivers the same count (its 8-frame workgroups sum in another order inside the loop)
        bat_mels, bat_audios = pkg.synthesize_batch(model, v, [[x] for x in ids], opts=o)
        for m2, a2 in zip(bat_mels, bat_audios):
            assert a2.shape == (n_out(256 * (m2.shape[1] - 1)),) and _rms(a2) > 0
    finally:
        v.close()


def _fit(y, f, Q, sl):
    """Least-squares amplitude and phase of a sine of frequency f in y[sl] at rate Q: (amplitude, max |residual|)."""
    m = np.arange(y.size, dtype=np.float64)[sl]
    A = np.stack([np.sin(2 * np.pi * f * m / Q), np.cos(2 * np.pi * f * m / Q)], axis=1)
    coef, *_ = np.linalg.lstsq(A, y[sl].astype(np.float64), rcond=None)
    return float(np.hypot(*coef)), float(np.max(np.abs(y[sl] - A @ coef)))


def test_a_sine_stays_a_sine(voc):
    """1 kHz through the hook stays a 1 kHz sine at the new rate (passband within 0.0001 dB: residual below 1e-4 of the
    amplitude away from the ends); 6 kHz at 8000, above the new Nyquist, comes out below -90 dB (the stopband is at -99 dB)."""
    n = np.arange(8192, dtype=np.float64)
    x1 = np.sin(2 * np.pi * 1000.0 * n / 22050.0 + 0.3).astype(np.float32)
    for Q in (8000, 48000):
        y = voc.resample(x1, Q)
        e = _edge(Q)
        amp, res = _fit(y, 1000.0, Q, slice(e, y.size - e))
        print("resample sine rate %d: amplitude %.7f, residual %.2e of it" % (Q, amp, res / amp))
        assert abs(amp - 1.0) <= 1e-4 and res <= 1e-4 * amp
    x6 = np.sin(2 * np.pi * 6000.0 * n / 22050.0 + 0.3).astype(np.float32)
    y = voc.resample(x6, 8000)
    e = _edge(8000)
    level = float(np.max(np.abs(y[e:-e])))
    print("resample 6 kHz at 8000: %.1f dB" % (20 * np.log10(max(level, 1e-30))))
    assert level < 10 ** (-90 / 20)
