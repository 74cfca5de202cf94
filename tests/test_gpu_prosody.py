"""GPU tests of the prosody stage (speaking rate and pitch on the magnitude between mel -> linear and the Griffin-Lim loop):
k_prosody against the fp64 restatement of its definition (tests/prosody_ref.py), the identity, exact zeros, the composition of
the entries, and the property the stage exists for -- the F0 of the audio follows `pitch` and ignores `rate`."""
import ctypes as C

import numpy as np
import pytest

import prosody_ref as pr
from conftest import synth_ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)
    yield v
    v.close()


@pytest.fixture(scope="module")
def voiced(voc):
    """The voiced signal (256 * 47 samples), its magnitude (513, 48) and log-mel (80, 48) from the GPU's own analysis."""
    y = pr.voiced_signal(256 * 47)
    S, mel = voc.analyze(y)
    for a in (y, S, mel):
        a.setflags(write=False)
    return y, S, mel


def middle_f0(audio):
    n = audio.size
    return pr.f0_autocorr(audio[n // 4 : 3 * n // 4])


CASES = [(1.0, 1.3), (0.5, 0.7), (2.0, 2.0), (1.25, 1.0), (4.0, 0.5), (0.25, 1.0)]


@pytest.mark.parametrize("F", [2, 3, 5, 37])
@pytest.mark.parametrize("rate, pitch", CASES)
def test_prosody_linear_matches_the_fp64_reference(pkg, voc, F, rate, pitch):
    """F = 2, 3, 5, 37 x (rate, pitch): reaches F' = 2, a partial last workgroup, more than one workgroup, warp positions beyond
    Nyquist (pitch < 1), an exact dyadic warp (pitch 2) and the interpolation alone (pitch 1).  Input: log-uniform over nine
    e-folds with 5 % exact zeros.  Metric: max |x - ref64| / max(ref64, log_floor) over all cells; bound 4 x d32 + 2e-5, d32 =
    the same metric of the float32 restatement (4: the room for another summation order; 2e-5: three times what some ten fp32
    roundings of a log value up to |ln 1e-5| = 11.5 through a radix-8 transform pair can give -- the transform is not scipy's).
    d32 is 1.5e-4 .. 1.8e-4 for the non-dyadic pitches (the fp32 warp position k / pitch), 1.5e-6 .. 2.3e-6 for pitch 2 and 0.5,
    and 0 .. 1.2e-7 for the interpolation alone.  The test prints err(gpu) and d32 of every case; no MI355X figures are recorded here yet."""
    S = pr.random_magnitude(F, seed=100 + F)
    ref = pr.prosody(S, rate, pitch)
    d32 = pr.rel_err(pr.prosody(S, rate, pitch, dtype=np.float32), ref)
    out = voc.prosody_linear(S, pkg.Prosody(rate=rate, pitch=pitch))
    assert out.shape == ref.shape == (513, pkg.prosody_frames(F, rate)) and out.dtype == np.float32 and np.all(np.isfinite(out))
    dg = pr.rel_err(out, ref)
    print("prosody F=%d F'=%d rate=%g pitch=%g: err(gpu) %.3e  d32 %.3e" % (F, out.shape[1], rate, pitch, dg, d32))
    assert dg <= 4.0 * d32 + 2e-5, (dg, d32)


def test_other_lifter_and_floor_follow_the_reference_too(pkg, voc):
    """The two remaining fields away from their defaults (lifter 255 = the widest the entry takes, a floor of 1e-3), same rule."""
    S = pr.random_magnitude(9, seed=77)
    for kw in (dict(lifter=255), dict(lifter=1), dict(log_floor=1e-3)):
        ref = pr.prosody(S, 0.8, 1.25, **kw)
        d32 = pr.rel_err(pr.prosody(S, 0.8, 1.25, dtype=np.float32, **kw), ref, kw.get("log_floor", 1e-5))
        out = voc.prosody_linear(S, pkg.Prosody(rate=0.8, pitch=1.25, **kw))
        dg = pr.rel_err(out, ref, kw.get("log_floor", 1e-5))
        print("prosody %s: err(gpu) %.3e  d32 %.3e" % (kw, dg, d32))
        assert out.shape == ref.shape and dg <= 4.0 * d32 + 2e-5, (kw, dg, d32)


def test_identity_returns_the_bits_of_the_plain_entries(pkg, voc, model):
    ident = pkg.Prosody()
    assert (ident.rate, ident.pitch) == (1.0, 1.0)
    S = pr.random_magnitude(37, seed=5)
    assert np.array_equal(voc.prosody_linear(S, ident), S)
    assert np.array_equal(voc.prosody_linear(S[:, :1], ident), S[:, :1])  # one frame is fine for the identity
    rng = np.random.default_rng(11)
    mel = (rng.uniform(-7.0, -1.0, size=(80, 40)) + 2.0 * np.sin(np.arange(40) / 5.0)[None, :]).astype(np.float32)
    voc.set_seed(3)
    assert np.array_equal(voc.infer_prosody(mel, ident), voc.infer(mel))
    ids = synth_ids(24, seed=2)
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    mel0, audio0 = pkg.synthesize(model, voc, ids, opts=opts)
    mel1, audio1 = pkg.synthesize(model, voc, ids, opts=opts, prosody=ident)
    assert np.array_equal(mel0, mel1) and np.array_equal(audio0, audio1) and audio0.size == 256 * 39


def test_zeros(pkg, voc):
    """Rate alone: a cell is exactly zero where the reference's is (both neighbours zero, or the one with all the weight), and
    nowhere else.  With a pitch change every cell is finite and positive (the floor enters the logarithm)."""
    S = pr.random_magnitude(37, seed=9).copy()
    S[:12, :] = 0.0  # whole bins, so that interpolated cells are zero too
    S[:, 20:23] = 0.0
    for rate in (1.25, 0.25, 2.0):
        out, ref = voc.prosody_linear(S, pkg.Prosody(rate=rate)), pr.prosody(S, rate, 1.0)
        assert (ref == 0).sum() > 12 * ref.shape[1] and np.array_equal(out == 0, ref == 0), rate
    for rate, pitch in ((1.0, 0.7), (1.25, 1.3), (1.0, 2.0)):
        out = voc.prosody_linear(S, pkg.Prosody(rate=rate, pitch=pitch))
        assert np.all(np.isfinite(out)) and np.all(out > 0), (rate, pitch)


def test_infer_prosody_is_the_composition_of_its_parts(pkg):
    """output_normalise = 0: infer_prosody(mel) == infer_linear(prosody_linear(mel_to_linear(mel)), iters = the handle's): the
    same kernels in the same order on the same seed stream.  The existing pair infer(mel) / infer_linear(mel_to_linear(mel)) is
    measured beside it and the new pair is held to the distance that one shows (0 if that pair is bit for bit, as its code says)."""
    rng = np.random.default_rng(11)
    mel = (rng.uniform(-7.0, -1.0, size=(80, 40)) + 2.0 * np.sin(np.arange(40) / 5.0)[None, :]).astype(np.float32)
    v = pkg.create_griffin_lim(iters=30, seed=5)
    try:
        v.set_opts(output_normalise=0)
        S = v.mel_to_linear(mel)
        d_pair = float(np.abs(v.infer(mel) - v.infer_linear(S)).max())
        for kw in (dict(rate=1.25), dict(pitch=0.8), dict(rate=0.7, pitch=1.3)):
            p = pkg.Prosody(**kw)
            whole = v.infer_prosody(mel, p)
            parts = v.infer_linear(v.prosody_linear(S, p))
            assert whole.shape == parts.shape == (256 * (pkg.prosody_frames(40, p.rate) - 1),)
            d = float(np.abs(whole - parts).max())
            print("composition %s: max |whole - parts| %.3e (the pair without prosody: %.3e)" % (kw, d, d_pair))
            assert d <= d_pair, (kw, d, d_pair)
        t = v.last_timings()
        assert t["mel_to_linear_ms"] > 0 and t["iterations_ms"] > 0
    finally:
        v.close()


@pytest.fixture(scope="module")
def f0_identity(voc, voiced):
    _, S, mel = voiced
    voc.set_seed(3)
    return middle_f0(voc.infer_linear(S, iters=30)), middle_f0(voc.infer(mel))


@pytest.mark.parametrize("rate, pitch", [(1.0, 0.8), (1.0, 1.25), (0.7, 1.3), (1.25, 1.0), (2.0, 1.0)])
def test_f0_follows_pitch_and_ignores_rate(pkg, voc, voiced, f0_identity, rate, pitch):
    """The voiced signal's own magnitude -> prosody_linear -> 30 iterations: 256 (F' - 1) samples, and the F0 of the middle
    half divided by the F0 of the identity run is within 4 % of `pitch` (a numpy prototype with another Griffin-Lim and another
    phase seed gave <= 2.1 %).
    The same chain through the fp32 CPU oracle's Griffin-Lim in place of the GPU's gives 0.8005, 1.2487, 1.2924 (0.6 % off
    1.3), 1.0035 and 1.0140; the test prints the GPU's ratios, no MI355X figures are recorded here yet."""
    _, S, _ = voiced
    p = pkg.Prosody(rate=rate, pitch=pitch)
    voc.set_seed(3)
    audio = voc.infer_linear(voc.prosody_linear(S, p), iters=30)
    assert audio.size == 256 * (pkg.prosody_frames(48, rate) - 1) and np.all(np.isfinite(audio))
    f0 = middle_f0(audio)
    print("rate %g pitch %g: F0 %.1f Hz, identity %.1f Hz, ratio %.4f" % (rate, pitch, f0, f0_identity[0], f0 / f0_identity[0]))
    assert abs(f0 / f0_identity[0] / pitch - 1.0) <= 0.04, (f0, f0_identity[0])


@pytest.mark.parametrize("pitch", [0.8, 1.25])
def test_f0_follows_pitch_through_the_mel_path(pkg, voc, voiced, f0_identity, pitch):
    """analyze -> log-mel -> infer_prosody: the same 4 % for the modest factors the mel bands still resolve (prototype: <= 1.5 %).
    Through the CPU oracle's mel -> linear and Griffin-Lim the ratios are 0.7985 and 1.2434; the test prints the GPU's."""
    _, _, mel = voiced
    voc.set_seed(3)
    audio = voc.infer_prosody(mel, pkg.Prosody(pitch=pitch))
    f0 = middle_f0(audio)
    print("mel path pitch %g: F0 %.1f Hz, identity %.1f Hz, ratio %.4f" % (pitch, f0, f0_identity[1], f0 / f0_identity[1]))
    assert audio.size == 256 * 47 and abs(f0 / f0_identity[1] / pitch - 1.0) <= 0.04, (f0, f0_identity[1])


def test_synthesize_with_a_rate_returns_tacotron2s_own_mel(pkg, voc, model):
    ids = synth_ids(24, seed=2)
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    mel0, _ = pkg.synthesize(model, voc, ids, opts=opts)
    mel1, audio = pkg.synthesize(model, voc, ids, opts=opts, prosody=pkg.Prosody(rate=1.25))
    assert mel0.shape == (80, 40) and np.array_equal(mel0, mel1)
    assert pkg.prosody_frames(40, 1.25) == 32 and audio.shape == (256 * 31,) and np.all(np.isfinite(audio)) and np.abs(audio).max() > 0


def test_bad_fields_are_rejected_on_a_live_handle(pkg, voc):
    S = np.ones((513, 3), dtype=np.float32)
    for kw in (dict(rate=0.2), dict(pitch=2.5), dict(lifter=0), dict(log_floor=0.0)):
        with pytest.raises(pkg.XdttsError) as e:
            voc.prosody_linear(S, pkg.Prosody(**kw))
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
        with pytest.raises(pkg.XdttsError) as e:
            voc.infer_prosody(np.zeros((80, 3), dtype=np.float32), pkg.Prosody(**kw))
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    with pytest.raises(pkg.XdttsError) as e:  # one frame, and not the identity
        voc.prosody_linear(S[:, :1], pkg.Prosody(pitch=1.25))
    assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    out, nf = np.zeros((513, 3), dtype=np.float32), C.c_size_t(7)
    st = pkg.lib.xdtts_griffinlim_prosody_linear(voc._h, None, 3, C.byref(pkg.Prosody()), out.ctypes.data_as(C.c_void_p), C.byref(nf))
    assert st == pkg.XDTTS_ERR_BAD_ARG and nf.value == 0
    # and the handle still works
    assert np.array_equal(voc.prosody_linear(S, pkg.Prosody()), S)
