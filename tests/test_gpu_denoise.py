"""GPU tests of the clean-up stage (spectral subtraction with a floor and a tone curve, the first stage of the magnitude chain):
k_noise_profile and k_denoise against xdtts_denoise_reference BIT FOR BIT on the crafted inputs (tests/denoise_ref.py), profile
mode and the selection alone, the stats, the ragged launch against the single one, the composition of the entries that honour
the handle's setting, batch against single on both engines, the sequence, synthesize and document entries, set-then-cleared
against never-set, argument errors on a live handle.  k_noise_profile has ONE route for every frame count, so
the frame counts are the issue's nine: one frame, fewer frames than a step of 32, exactly and around two half-steps, more than
one step, and 300 (the unrolled loop and its tail).  Inputs hold no subnormals: the kernels keep them by default, nothing here
relies on it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import denoise_ref as dr
from conftest import synth_ids

pytestmark = pytest.mark.gpu

FS = (1, 2, 3, 15, 16, 17, 64, 65, 300)
QS = (0.0, 0.1, 0.5, 1.0)
TONE = [(300.0, -12.0), (1000.0, 3.0), (3400.0, 0.0)]


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)
    yield v
    v.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _input(F):
    S = dr.crafted(F)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _profile():
    p = dr.noise(dr.crafted(40, seed=1), 0.5)
    p.setflags(write=False)
    return p


def _mel(F, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 2.0 * np.sin(np.arange(F) / 5.0)[None, :]).astype(np.float32)


# ---- 1. the stage alone == the serial reference, bit for bit -----------------------------------------------------------------------

@pytest.mark.parametrize("F", FS)
def test_stage_alone_equals_the_reference_bit_for_bit(pkg, voc, F):
    """Every F x q in {0, 0.1, 0.5, 1}, strength 2, floor -20 dB, on the crafted 513-bin input (a constant column, four distinct
    values, more than r + 1 exact zeros, a nextafter chain, values that differ in the top byte only, the lone bin 512): samples
    and stats equal xdtts_denoise_reference's; the selection alone equals the reference's order statistic."""
    S = _input(F)
    for q in QS:
        d = pkg.Denoise(strength=2.0, quantile=q)
        want, wst = pkg.denoise_reference(S, d)
        got = voc.denoise_linear(S, d)
        st = voc.last_denoise()
        assert got.shape == (513, F) and np.array_equal(_bits(got), _bits(want)), (F, q, int(np.count_nonzero(_bits(got) != _bits(want))))
        assert len(st) == 1 and st[0].astuple() == wst.astuple() == (513 * F, wst.floored, pkg.denoise_rank(F, q), 0), (F, q)
        N = voc.noise_profile(S, q)
        assert np.array_equal(_bits(N), _bits(dr.noise(S, q))), (F, q)
        assert N[0] == np.float32(0.125) and (F < 3 or q == 1.0 or N[2] == 0.0)


@pytest.mark.parametrize("F", (1, 17, 300))
def test_other_settings_equal_the_reference(pkg, voc, F):
    """The extreme strengths and floors, and subtraction with a tone curve behind it."""
    S = _input(F)
    for d in (pkg.Denoise(strength=16.0, quantile=1.0, floor_db=-80.0), pkg.Denoise(strength=0.5, quantile=0.1, floor_db=0.0),
              pkg.Denoise(strength=1.0, quantile=0.5, floor_db=-6.0, tone=TONE)):
        want, wst = pkg.denoise_reference(S, d)
        got = voc.denoise_linear(S, d)
        assert np.array_equal(_bits(got), _bits(want)), (F, d.astuple())
        assert voc.last_denoise()[0].astuple() == wst.astuple()
        assert np.all(np.isfinite(got)) and np.all(got >= 0) and np.all(got[S == 0] == 0)


def test_profile_mode_and_the_selection_alone(pkg, voc):
    """A caller's profile takes the selection's place: equal to the reference; and the profile noise_profile returns, handed
    back in, gives the bits of the run that selected it itself."""
    S = _input(65)
    d = pkg.Denoise(strength=2.0, quantile=0.5, floor_db=-30.0)
    want, wst = pkg.denoise_reference(S, d, _profile())
    got = voc.denoise_linear(S, d, _profile())
    assert np.array_equal(_bits(got), _bits(want)) and wst.profiled == 1 and wst.rank == 0
    assert voc.last_denoise()[0].astuple() == wst.astuple()
    own = voc.noise_profile(S, 0.5)
    a, b = voc.denoise_linear(S, d, own), voc.denoise_linear(S, d)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(b), _bits(pkg.denoise_reference(S, d)[0]))


def test_tone_alone(pkg, voc):
    """strength 0, three points: no selection, no gain -- S * E, equal to the reference; the stats count no floored cell."""
    S = _input(17)
    d = pkg.Denoise(strength=0.0, tone=TONE)
    want, wst = pkg.denoise_reference(S, d)
    got = voc.denoise_linear(S, d)
    assert np.array_equal(_bits(got), _bits(want)) and wst.astuple() == (513 * 17, 0, 0, 0) == voc.last_denoise()[0].astuple()
    E = pkg.denoise_tone(d)
    assert np.array_equal(_bits(got), _bits((S * E[:, None]).astype(np.float32)))


def test_identity_returns_the_input_bits(pkg, voc):
    S = _input(16).copy()
    S[7, 3] = np.float32("nan")
    for d in (pkg.Denoise(), pkg.Denoise(quantile=0.9, floor_db=-70.0), pkg.Denoise(tone=[(100.0, 0.0), (5000.0, 0.0)])):
        assert np.array_equal(_bits(voc.denoise_linear(S, d)), _bits(S))
    d, prof = voc.get_denoise()
    assert d.astuple() == pkg.Denoise().astuple() and prof is None  # a fresh handle holds the default


# ---- 2. batch == single, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (3, 0, 4, 2, 1)])
def test_ragged_launch_equals_the_single_launch(pkg, voc, order):
    """Fs = [1, 5, 2, 300, 64] under the identity, a tone alone, two quantiles and a subtraction with a tone, without and with a
    shared profile, in two orders: every S_outs[u] is denoise_linear of that utterance alone -- the order statistic is over the
    frames of the utterance alone, never a neighbour's.  The stats come in the caller's order."""
    Fs = [1, 5, 2, 300, 64]
    ds = [pkg.Denoise(), pkg.Denoise(tone=TONE), pkg.Denoise(strength=2.0, quantile=1.0), pkg.Denoise(strength=1.5, quantile=0.1, floor_db=-12.0),
          pkg.Denoise(strength=2.0, quantile=0.5, tone=[(1000.0, 3.0)])]
    Ss = [dr.crafted(F, seed=40 + u) for u, F in enumerate(Fs)]
    for prof in (None, _profile()):
        single, stats = [], []
        for S, d in zip(Ss, ds):
            single.append(voc.denoise_linear(S, d, prof))
            stats.append(pkg.denoise_reference(S, d, prof)[1].astuple())
        assert np.array_equal(_bits(single[0]), _bits(Ss[0]))
        outs = voc.denoise_linear_batch([Ss[u] for u in order], [ds[u] for u in order], prof)
        got = [s.astuple() for s in voc.last_denoise()]
        for k, u in enumerate(order):
            assert outs[k].shape == (513, Fs[u]) and np.array_equal(_bits(outs[k]), _bits(single[u])), (order, u, prof is not None)
            assert np.array_equal(_bits(outs[k]), _bits(pkg.denoise_reference(Ss[u], ds[u], prof)[0]))
        assert got == [stats[u] for u in order]
    # a batch of identities alone touches nothing and returns the inputs' bits
    same = voc.denoise_linear_batch(Ss[:3], [pkg.Denoise()] * 3)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(same, Ss))


# ---- 3. composition -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase_init", [0, 1])
def test_infer_under_a_denoise_is_the_composition_of_its_parts(pkg, phase_init):
    """output_normalise = 0, a 40-frame mel, a setting with subtraction and tone: infer(mel) == infer_linear(denoise_linear(
    mel_to_linear(mel))), and the same with a prosody and a timbre behind it, each held to the distance the plain pair infer /
    infer_linear shows here with the setting off (the rule of test_infer_under_a_timbre_is_the_composition_of_its_parts)."""
    mel = _mel(40)
    d = pkg.Denoise(strength=2.0, quantile=0.5, tone=TONE)
    t = pkg.Timbre(vtl=1.25, breath=0.3, seed=4)
    p = pkg.Prosody(rate=0.7, pitch=1.3)
    v = pkg.create_griffin_lim(iters=30, seed=5)
    try:
        v.set_opts(output_normalise=0, batch_shape=4)
        v.set_phase_init(phase_init)
        S = v.mel_to_linear(mel)
        off = v.infer(mel)
        d_pair = float(np.abs(off - v.infer_linear(S)).max())
        v.set_denoise(d)
        Sc = v.denoise_linear(S, d)
        assert np.array_equal(_bits(Sc), _bits(pkg.denoise_reference(S, d)[0]))
        whole, parts = v.infer(mel), v.infer_linear(Sc)
        dist = float(np.abs(whole - parts).max())
        print("composition phase_init %d: max |infer - parts| %.3e (the pair without the stage: %.3e)" % (phase_init, dist, d_pair))
        assert whole.shape == parts.shape == (256 * 39,) and dist <= d_pair, (dist, d_pair)
        assert not np.array_equal(whole, off)
        assert v.last_denoise() == []  # (infer_linear does not run the stage and cleared the stats)
        v.infer(mel)
        assert [s.astuple() for s in v.last_denoise()] == [pkg.denoise_reference(S, d)[1].astuple()]
        v.set_timbre(t)
        whole = v.infer_prosody(mel, p)
        parts = v.infer_linear(v.timbre_linear(v.prosody_linear(Sc, p), t))
        dist = float(np.abs(whole - parts).max())
        print("composition phase_init %d, prosody and timbre behind: max |infer_prosody - parts| %.3e (pair: %.3e)" % (phase_init, dist, d_pair))
        assert whole.shape == parts.shape == (256 * (pkg.prosody_frames(40, p.rate) - 1),) and dist <= d_pair, (dist, d_pair)
        # infer_linear and the other stages' hooks do not honour the setting
        assert np.array_equal(v.prosody_linear(S, p), v.prosody_linear(S, p))
        v.set_timbre(None)
        assert not np.array_equal(v.infer_linear(S), v.infer(mel))
    finally:
        v.close()


def test_the_tracker_sees_the_cleaned_magnitude(pkg, voc):
    """infer_pitch_target's F0 stats == the tracker's on denoise_linear(S), bit for bit: what the tracker finds (n_frames, n_voiced,
    median, min, max) against f0_linear, and the whole struct -- n_clamped and base_ratio are the target's, which f0_linear does
    not take (an identity target runs no tracker at all) -- against the target's own hook on the cleaned magnitude."""
    mel = _mel(40, seed=12)
    d = pkg.Denoise(strength=2.0, quantile=0.5)
    tg = pkg.PitchTarget(factor=1.1)
    try:
        S = voc.mel_to_linear(mel)
        Sc = voc.denoise_linear(S, d)
        want = bytes(voc.f0_linear(Sc)[3])
        plain = bytes(voc.f0_linear(S)[3])
        whole = bytes(voc.pitch_target_linear(Sc, tg)[2])
        voc.set_denoise(d)
        voc.infer_pitch_target(mel, tg)
        got = voc.last_f0()
        assert len(got) == 1 and bytes(got[0]) == whole
        found = lambda b: b[:8] + b[12:24]  # n_frames, n_voiced | median_hz, min_hz, max_hz
        assert found(bytes(got[0])) == found(want) and got[0].n_frames == 40
        assert len(voc.last_denoise()) == 1
        print("f0 stats under the stage differ from the plain ones: %s" % (want != plain))
    finally:
        voc.set_denoise(None)


# ---- 4. batch against single, both engines ----------------------------------------------------------------------------------------

def _batch_equals_single(pkg):
    mel = _mel(40)
    mels = [mel[:, :5], mel, mel[:, 20:32]]
    v = pkg.create_griffin_lim(iters=30, seed=5)
    try:
        v.set_opts(batch_shape=4)
        v.set_denoise(pkg.Denoise(strength=2.0, quantile=0.5, tone=TONE))
        single, stats = [], []
        for m in mels:
            single.append(v.infer(m).copy())
            stats += [s.astuple() for s in v.last_denoise()]
        got = v.infer_batch(mels)
        for a, b in zip(got, single):
            assert a.shape == b.shape and np.array_equal(a, b)
        assert [s.astuple() for s in v.last_denoise()] == stats and len(stats) == 3
        assert [s[0] for s in stats] == [513 * 5, 513 * 40, 513 * 12]
    finally:
        v.close()


def test_infer_batch_equals_single_under_the_stage(pkg):
    _batch_equals_single(pkg)


def test_infer_batch_equals_single_on_the_launch_per_iteration_engine(pkg):
    os.environ["XDTTS_GL"] = "launch"
    try:
        _batch_equals_single(pkg)
    finally:
        del os.environ["XDTTS_GL"]


# ---- 5. through the model -----------------------------------------------------------------------------------------------------

def test_sequence_synthesize_and_document_under_the_stage(pkg, voc, model):
    """synthesize_sequence of two 24-id utterances under the setting == two synthesize calls under it, bit for bit; the mels are
    Tacotron2's own (those of the run without the stage); synthesize_document of the same two as fp32 at level 0 == join of the two
    audios; the stats of the sequence come utterance by utterance."""
    ids = [synth_ids(24, seed=2), synth_ids(24, seed=3)]
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    voc.set_seed(3)
    voc.set_denoise(None)
    plain = [pkg.synthesize(model, voc, x, opts=opts) for x in ids]
    assert voc.last_denoise() == []
    try:
        voc.set_denoise(pkg.Denoise(strength=2.0, quantile=0.5, tone=TONE))
        single, stats = [], []
        for x in ids:
            single.append(pkg.synthesize(model, voc, x, opts=opts))
            stats += [s.astuple() for s in voc.last_denoise()]
        assert len(stats) == 2 and all(s[0] == 513 * 40 for s in stats)
        mels, audios = pkg.synthesize_sequence(model, voc, ids, opts=opts)
        assert [s.astuple() for s in voc.last_denoise()] == stats
        for u in range(2):
            assert np.array_equal(mels[u], plain[u][0]) and np.array_equal(single[u][0], plain[u][0])
            assert audios[u].shape == (256 * 39,) and np.array_equal(audios[u], single[u][1])
            assert not np.array_equal(audios[u], plain[u][1])
        gaps = [100, 2205, 0]
        so = pkg.StreamOpts(format=0, level=0)
        dmels, stream, offs = pkg.synthesize_document(model, voc, ids, gaps=gaps, stream_opts=so, opts=opts)
        want, woffs = voc.join(audios, gaps, opts=so)
        assert offs == woffs and stream.dtype == np.float32 and np.array_equal(stream, want)
        assert all(np.array_equal(dmels[u], plain[u][0]) for u in range(2))
    finally:
        voc.set_denoise(None)


def test_set_then_cleared_is_never_set(pkg, model):
    """infer, infer_prosody, infer_batch and synthesize on a handle whose setting (with a profile) was set, used and cleared ==
    the same on a handle that never had it, bit for bit; the getter returns what was set."""
    never = pkg.create_griffin_lim(iters=30, seed=3)
    was = pkg.create_griffin_lim(iters=30, seed=3)
    mel = _mel(40)
    p = pkg.Prosody(rate=1.25, pitch=0.8)
    ids = synth_ids(24, seed=2)
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)

    def run(v):
        v.set_seed(3)
        return [v.infer(mel), v.infer_prosody(mel, p), v.infer_batch([mel, mel[:, :12]])[1]] + list(pkg.synthesize(model, v, ids, opts=opts))

    try:
        d = pkg.Denoise(strength=3.0, quantile=0.25, floor_db=-30.0, tone=TONE)
        prof = np.full(513, 1e-3, dtype=np.float32)
        was.set_denoise(d, prof)
        got, gp = was.get_denoise()
        assert got.astuple() == d.astuple() and np.array_equal(gp, prof)
        on = run(was)
        assert [s.astuple()[2:] for s in was.last_denoise()] == [(0, 1)]  # profiled, no selection
        fresh = run(never)
        assert not np.array_equal(on[0], fresh[0]) and np.array_equal(on[3], fresh[3])  # the mel is Tacotron2's own
        was.set_denoise(None)
        got, gp = was.get_denoise()
        assert got.astuple() == pkg.Denoise().astuple() and gp is None
        for a, b in zip(run(was), fresh):
            assert a.shape == b.shape and np.array_equal(a, b)
        assert was.last_denoise() == []
    finally:
        never.close()
        was.close()


# ---- 6. argument errors -------------------------------------------------------------------------------------------------------

def test_bad_fields_are_rejected_on_a_live_handle(pkg, voc):
    S = np.ones((513, 3), dtype=np.float32)
    keep = pkg.Denoise(strength=1.5, quantile=0.25, floor_db=-12.0, tone=[(500.0, -3.0)])
    prof = np.full(513, 2e-3, dtype=np.float32)
    voc.set_denoise(keep, prof)
    try:
        bads = [pkg.Denoise(**{f: x}) for f, x in (("strength", -1.0), ("strength", 17.0), ("strength", float("nan")), ("quantile", 1.5),
                                                   ("quantile", float("inf")), ("floor_db", -81.0), ("floor_db", 1.0), ("n_tone", 9))]
        names = ["strength"] * 3 + ["quantile"] * 2 + ["floor_db"] * 2 + ["n_tone"]
        bads += [pkg.Denoise(tone=[(200.0, 0.0), (100.0, 0.0)]), pkg.Denoise(tone=[(12000.0, 0.0)]), pkg.Denoise(tone=[(100.0, 21.0)])]
        names += ["tone_hz", "tone_hz", "tone_db"]
        for field, bad in zip(names, bads):
            for call in (lambda: voc.set_denoise(bad), lambda: voc.denoise_linear(S, bad)):
                with pytest.raises(pkg.XdttsError) as e:
                    call()
                assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and field in str(e.value), (field, str(e.value))
            got, gp = voc.get_denoise()
            assert got.astuple() == keep.astuple() and np.array_equal(gp, prof)  # a failed set leaves the setting as it was
        badp = prof.copy()
        badp[5] = np.nan
        with pytest.raises(pkg.XdttsError) as e:
            voc.set_denoise(keep, badp)
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and "profile[5]" in str(e.value)
        assert np.array_equal(voc.get_denoise()[1], prof)
        with pytest.raises(pkg.XdttsError) as e:
            voc.denoise_linear_batch([S, S, S], [pkg.Denoise(), pkg.Denoise(strength=99.0), pkg.Denoise()])
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and "utterance 1" in str(e.value) and "strength" in str(e.value)
        out = np.zeros((513, 3), dtype=np.float32)
        good = pkg.Denoise(strength=2.0)
        assert pkg.lib.xdtts_griffinlim_denoise_linear(voc._h, None, 3, C.byref(good), None, out.ctypes.data_as(C.c_void_p)) == pkg.XDTTS_ERR_BAD_ARG
        assert pkg.lib.xdtts_griffinlim_denoise_linear(voc._h, S.ctypes.data_as(C.c_void_p), 0, C.byref(good), None, out.ctypes.data_as(C.c_void_p)) == pkg.XDTTS_ERR_BAD_ARG
        # and the handle still works: one frame is enough for the stage
        one = voc.denoise_linear(S[:, :1], good)
        assert np.array_equal(_bits(one), _bits(pkg.denoise_reference(S[:, :1], good)[0]))
    finally:
        voc.set_denoise(None)
