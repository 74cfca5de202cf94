"""GPU tests of the pitch tracker and of pitch targets (k_f0_frames, k_f0_track): the per-frame stage against the fp64
restatement of its definition (tests/f0_ref.py), the utterance stage against the host reference bit for bit, the ragged form
against the single one, the application against contour_ref fed the device's own ratios, the identity, the composition of the
entries, and the property the feature exists for -- the median F0 of the audio lands on the target."""
import numpy as np
import pytest

import contour_ref as cr
import f0_ref as fr
import gpu_f0_cases as gc
import prosody_ref as pr
from conftest import synth_ids
from test_f0_cpu import TARGETS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)
    v.set_opts(batch_shape=4)  # the single call's split into workgroups: a batch's audio is the single call's bit for bit
    yield v
    v.close()


@pytest.fixture(scope="module")
def voiced(pkg):
    out = gc.voiced_magnitudes(pkg)
    for S in out.values():
        S.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def frame_refs(voiced):
    """name -> (S, the fp64 restatement, the fp32 one), computed once."""
    return {name: (S, fr.frames(S, fr.opts(), np.float64), fr.frames(S, fr.opts(), np.float32)) for name, S in gc.frame_cases(voiced).items()}


def target_of(pkg, t):
    return pkg.PitchTarget(mode=t[0], value=t[1], range=t[2])


def stats_bits(s):
    return s.bits()


NAMES = ["random%d" % F for F in gc.FRAMES] + ["voiced140true", "voiced140mel", "voiced220true", "voiced220mel", "zero37"]


@pytest.mark.parametrize("name", NAMES)
def test_frame_stage_matches_the_fp64_reference(pkg, voc, frame_refs, name):
    """_f0_linear on random magnitudes (5 % exact zeros) at F = 1, 2, 5, 37, 64, on the four voiced magnitudes (F = 64) and on an
    all-zero S.  strength within 4 x d32 + 2e-5 of the fp64 reference, d32 = the fp32 restatement's own distance on the
    cepstrum (the bound of test_gpu_contour.py); n* equal to the reference's except where a comparison of the rule lies within
    that bound of its threshold in the fp64 cepstrum -- those frames are counted and capped at 2 % of the case (the fp32
    restatement alone stays inside the cap: tests/test_f0_cpu.py); where n* agrees, raw within the same bound, relative."""
    S, (n64, raw64, s64, c64), (n32, raw32, s32, c32) = frame_refs[name]
    F = S.shape[1]
    d32 = float(np.max(np.abs(c32[:, :513].astype(np.float64) - c64[:, :513])))
    bound = 4.0 * d32 + 2e-5
    raw, strength, f0, stats = voc.f0_linear(S)
    assert raw.shape == strength.shape == f0.shape == (F,) and np.all(np.isfinite(raw)) and np.all(raw > 0)
    # the device returns raw, not n*: 22050 / raw = n* + p with |p| <= 0.5, so n* is the nearest integer of the period -- or, with
    # p at its clamp, the one the reference's n* reaches too
    period = 22050.0 / raw.astype(np.float64)
    same = (np.rint(period).astype(np.int64) == n64) | (np.abs(period - n64) <= 0.5 + 1e-4)
    amb = fr.ambiguous(c64, fr.opts(), bound)
    differ = ~same
    print("f0 frames %s F=%d: d32 %.3e, bound %.3e, |strength - ref| %.3e, n* differs in %d frame(s), %d ambiguous" % (
        name, F, d32, bound, float(np.max(np.abs(strength.astype(np.float64) - s64)[~differ], initial=0.0)), int(differ.sum()), int(amb.sum())))
    assert not np.any(differ & ~amb), (name, np.nonzero(differ & ~amb)[0][:8])
    assert differ.sum() <= 0.02 * F, (name, int(differ.sum()))
    ok = ~differ
    assert np.all(np.abs(strength.astype(np.float64) - s64)[ok] <= bound), name
    rel = np.abs(raw.astype(np.float64) / raw64 - 1.0)[ok]
    print("   raw: max relative distance on %d agreeing frame(s) %.3e" % (int(ok.sum()), rel.max(initial=0.0)))
    assert np.all(rel <= bound), (name, rel.max(), bound)
    if name == "zero37":
        assert stats.n_voiced == 0 and np.all(f0 == 0) and np.all(strength == 0)


UTT_F = [1, 2, 5, 6, 37, 64]


def test_utterance_stage_equals_the_host_reference_bit_for_bit(pkg, voc, voiced):
    """The device's own raw / strength through xdtts_f0_track_reference: f0, voiced flags and every stats field bit for bit,
    ratio within 2 ulp of the fp32 restatement.  The utterances: random magnitudes at threshold 0 (every frame voiced) and at
    0.05 (a mix), a voiced magnitude, an all-zero one, and a magnitude whose frames repeat in blocks of 7 (ties)."""
    rep = np.repeat(pr.random_magnitude(10, seed=9), 7, axis=1)[:, :64]
    mags = [pr.random_magnitude(F, seed=40 + F) for F in UTT_F] + [voiced[(140.0, "mel")], np.zeros((513, 5), np.float32), rep]
    m2 = [S for S in mags if S.shape[1] >= 2]  # (a target that is not the identity takes two frames)
    for thr in (0.0, 0.05, 0.2):
        o = pkg.F0Opts(threshold=thr)
        for target in TARGETS[:6]:
            outs, ratios, stats = voc.pitch_target_linear_batch(m2, [target_of(pkg, target)] * len(m2), opts=o)
            raws, strengths, f0s, _ = voc.f0_linear_batch(m2, opts=o)
            for u, (raw, strength) in enumerate(zip(raws, strengths)):
                f0_ref, ratio_ref, st_ref = pkg.f0_track_reference(raw, strength, opts=o, target=target_of(pkg, target))
                assert np.array_equal(f0s[u].view(np.uint32), f0_ref.view(np.uint32)), (thr, target, u)
                assert stats_bits(stats[u]) == stats_bits(st_ref), (thr, target, u, stats[u].astuple(), st_ref.astuple())
                assert np.abs(ratios[u].view(np.int32).astype(np.int64) - ratio_ref.view(np.int32).astype(np.int64)).max() <= 2, (thr, target, u)
                rf0, voiced_ref, rratio, rs = fr.track(raw, strength, fr.opts(threshold=thr), target, np.float32)
                assert np.array_equal(f0s[u] > 0, voiced_ref) and np.abs(ratios[u].view(np.int32).astype(np.int64) - rratio.view(np.int32).astype(np.int64)).max() <= 2
    # one frame: the tracker alone takes it
    raw, strength, f0, st = voc.f0_linear(mags[0], opts=pkg.F0Opts(threshold=0.0))
    f0_ref, _, st_ref = pkg.f0_track_reference(raw, strength, opts=pkg.F0Opts(threshold=0.0))
    assert np.array_equal(f0, f0_ref) and stats_bits(st) == stats_bits(st_ref) and st.n_voiced == 1


def test_utterance_stage_at_full_size(pkg, voc):
    """F = 16384 at threshold 0: every frame is voiced and the selection runs at full size; twice, for the same bits."""
    S = pr.random_magnitude(16384, seed=3)
    o = pkg.F0Opts(threshold=0.0)
    raw, strength, f0, st = voc.f0_linear(S, opts=o)
    f0_ref, _, st_ref = pkg.f0_track_reference(raw, strength, opts=o)
    assert st.n_voiced == 16384 and st.n_frames == 16384
    assert np.array_equal(f0.view(np.uint32), f0_ref.view(np.uint32)) and stats_bits(st) == stats_bits(st_ref)
    raw2, strength2, f02, st2 = voc.f0_linear(S, opts=o)
    assert np.array_equal(raw, raw2) and np.array_equal(strength, strength2) and np.array_equal(f0, f02) and stats_bits(st) == stats_bits(st2)
    out, ratio, st3 = voc.pitch_target_linear(S, pkg.PitchTarget(hz=150.0, range=0.5), opts=o)
    _, ratio_ref, st3_ref = pkg.f0_track_reference(raw, strength, opts=o, target=pkg.PitchTarget(hz=150.0, range=0.5))
    assert stats_bits(st3) == stats_bits(st3_ref) and out.shape == (513, 16384) and np.all(np.isfinite(out))
    assert np.abs(ratio.view(np.int32).astype(np.int64) - ratio_ref.view(np.int32).astype(np.int64)).max() <= 2


BATCH_F = (1, 5, 64, 37)


def test_ragged_forms_equal_the_single_entries(pkg, voc, voiced):
    """_f0_linear_batch and _pitch_target_linear_batch on F = 1, 5, 64, 37 in both orders: np.array_equal on every output and on
    the stats.  The F = 1 utterance carries the identity target (a target that is not the identity takes two frames, as a
    contour does), the F = 5 one is all zero (n_voiced = 0, every ratio 1, copied), F = 64 is the 140 Hz voice under an
    absolute target and F = 37 a random magnitude under a range with a caller's contour."""
    mags = [pr.random_magnitude(1, seed=61), np.zeros((513, 5), np.float32), voiced[(140.0, "mel")], pr.random_magnitude(37, seed=62)]
    targets = [pkg.PitchTarget(), pkg.PitchTarget(hz=200.0), pkg.PitchTarget(hz=120.0, range=1.5), pkg.PitchTarget(factor=1.0, range=2.0)]
    contours = [None, None, None, pkg.ProsodyContour(cr.CONTOURS["ramp"])]
    o = pkg.F0Opts(threshold=0.05)
    single_f0 = [voc.f0_linear(S, opts=o) for S in mags]
    for order in (slice(None), slice(None, None, -1)):
        raws, strengths, f0s, stats = voc.f0_linear_batch(mags[order], opts=o)
        for u, one in zip(range(4)[order], zip(raws, strengths, f0s, stats)):
            for k in range(3):
                assert np.array_equal(one[k], single_f0[u][k]), (u, k)
            assert stats_bits(one[3]) == stats_bits(single_f0[u][3]), u
    single = [voc.pitch_target_linear(S, t, c, opts=o) for S, t, c in zip(mags, targets, contours)]
    for order in (slice(None), slice(None, None, -1)):
        outs, ratios, stats = voc.pitch_target_linear_batch(mags[order], targets[order], contours[order], opts=o)
        for u, (out, ratio, st) in zip(range(4)[order], zip(outs, ratios, stats)):
            assert out.shape == single[u][0].shape and np.array_equal(out, single[u][0]), u
            assert np.array_equal(ratio, single[u][1]) and stats_bits(st) == stats_bits(single[u][2]), u
    assert np.array_equal(single[0][0], mags[0]) and np.all(single[0][1] == 1.0)  # the identity inside a mixed batch: copied
    assert single[1][2].n_voiced == 0 and np.all(single[1][1] == 1.0) and np.array_equal(single[1][0], mags[1])
    assert single[3][0].shape == (513, cr.frames(cr.CONTOURS["ramp"], 37)) and single[2][2].n_voiced > 50


def f0_of(S):
    """(f0, voiced) of a magnitude by the fp64 restatement at the default options."""
    _, raw, strength, _ = fr.frames(S, fr.opts(), np.float64)
    f0, voiced, _, _ = fr.track(raw.astype(np.float32), strength.astype(np.float32), fr.opts())
    return f0, voiced


@pytest.mark.parametrize("f0,kind", [(140.0, "true"), (140.0, "mel"), (220.0, "true"), (220.0, "mel")])
def test_application_follows_the_reference_and_lands_on_the_target(pkg, voc, voiced, f0, kind):
    """_pitch_target_linear with hz = 0.85 / 1.15 x f0, {2, 1, 0}, {2, 1, 2} and {1, 1.1 f0, 0.5}: S_out against contour_ref's
    stage fed the device's own ratios, within the bound of test_gpu_contour.py; the F0 of S_out, from the fp64 restatement, meets
    the median and excursion conditions of tests/test_f0_cpu.py."""
    S = voiced[(f0, kind)]
    F = S.shape[1]
    est, v_in = f0_of(S)
    e_in = fr.excursion_cents(est, v_in)
    c, one, gain = fr.rate1_table(F)
    for target in ((1, 0.85 * f0, 1.0), (1, 1.15 * f0, 1.0), (2, 1.0, 0.0), (2, 1.0, 2.0), (1, 1.1 * f0, 0.5)):
        out, ratio, st = voc.pitch_target_linear(S, target_of(pkg, target))
        pitch = fr.table_pitch(one, ratio)
        ref = fr.apply_table(S, c, pitch, gain)
        r32 = fr.apply_table(S, c, pitch, gain, dtype=np.float32)
        dg, d32 = pr.rel_err(out, ref), pr.rel_err(r32, ref)
        e2, v2 = f0_of(out)
        med = fr.lower_median(e2[4 : F - 4][v2[4 : F - 4]])
        x = fr.excursion_cents(e2, v2)
        print("target %s on %s %g Hz: err(gpu) %.3e d32 %.3e; median %.2f Hz, excursion %.1f cents (input %.1f), clamped %d" % (
            target, kind, f0, dg, d32, med, x, e_in, st.n_clamped))
        assert out.shape == ref.shape and np.all(np.isfinite(out)) and dg <= 4.0 * d32 + 2e-5, (target, dg, d32)
        assert st.n_voiced >= 0.9 * F
        if target[0] == 1 and target[2] == 1.0:
            assert abs(med / target[1] - 1.0) <= 0.01, (target, med)
        if target == (2, 1.0, 0.0):
            assert x <= e_in / 3.0, (x, e_in)
        if target == (2, 1.0, 2.0):
            assert 1.7 * e_in <= x <= 2.4 * e_in, (x, e_in)


def test_application_with_a_callers_contour_keeps_its_rate_and_gain(pkg, voc, voiced):
    """A rate ramp 1 -> 1.5 with gain 0.5: F' is the contour's, and so are the gains -- the output is half the output of the same
    request with gain 1, bit for bit (a power of two), and equals contour_ref's stage on the table whose pitches are the
    contour's times the device's ratios."""
    S = voiced[(140.0, "mel")]
    pts = [(0.0, 1.0, 1.0, 0.5), (1.0, 1.5, 1.0, 0.5)]
    pts1 = [(0.0, 1.0, 1.0, 1.0), (1.0, 1.5, 1.0, 1.0)]
    t = pkg.PitchTarget(hz=160.0)
    out, ratio, st = voc.pitch_target_linear(S, t, pkg.ProsodyContour(pts))
    out1, ratio1, _ = voc.pitch_target_linear(S, t, pkg.ProsodyContour(pts1))
    Fp = cr.frames(pts, 64)
    assert out.shape == (513, Fp) and Fp < 64 and np.array_equal(ratio, ratio1) and np.array_equal(out, np.float32(0.5) * out1)
    c, pt, gn = cr.table(pts, 64)
    ref = fr.apply_table(S, c, fr.table_pitch(pt, ratio), gn)
    r32 = fr.apply_table(S, c, fr.table_pitch(pt, ratio), gn, dtype=np.float32)
    dg, d32 = pr.rel_err(out, ref), pr.rel_err(r32, ref)
    print("target 160 Hz under a rate ramp: F' %d, err(gpu) %.3e d32 %.3e" % (Fp, dg, d32))
    assert dg <= 4.0 * d32 + 2e-5, (dg, d32)


@pytest.fixture(scope="module")
def mel40():
    rng = np.random.default_rng(11)
    mel = (rng.uniform(-7.0, -1.0, size=(80, 40)) + 2.0 * np.sin(np.arange(40) / 5.0)[None, :]).astype(np.float32)
    mel.setflags(write=False)
    return mel


def test_identity_returns_the_bits_of_the_plain_entries(pkg, voc, mel40):
    """{0, 1, 1} and {2, 1, 1}: the bits of infer, and with a contour of infer_contour; nothing is tracked (last_f0 is empty).
    And the engine after the stage: a plain infer behind a target call returns the bits it returned before."""
    voc.set_seed(3)
    plain = voc.infer(mel40)
    step = pkg.ProsodyContour(cr.CONTOURS["step"])
    with_contour = voc.infer_contour(mel40, step)
    for t in (pkg.PitchTarget(), pkg.PitchTarget(factor=1.0)):
        assert np.array_equal(voc.infer_pitch_target(mel40, t), plain) and voc.last_f0() == []
        assert np.array_equal(voc.infer_pitch_target(mel40, t, step), with_contour) and voc.last_f0() == []
        got = voc.infer_batch_pitch_target([mel40, mel40], [t, t], [None, step])
        assert np.array_equal(got[0], plain) and np.array_equal(got[1], with_contour) and voc.last_f0() == []
    moved = voc.infer_pitch_target(mel40, pkg.PitchTarget(factor=1.2, range=0.5), opts=pkg.F0Opts(threshold=0.0))
    assert moved.shape == plain.shape and not np.array_equal(moved, plain) and len(voc.last_f0()) == 1 and voc.last_f0()[0].n_frames == 40
    assert np.array_equal(voc.infer(mel40), plain) and voc.last_f0() == []  # nothing of the stage lingers in the handle
    assert np.array_equal(voc.infer_contour(mel40, step), with_contour)


def test_batched_vocoder_equals_the_single_entry(pkg, voc):
    """infer_batch_pitch_target(...)[u] is infer_pitch_target for that utterance alone, bit for bit with batch_shape = 4, in
    both orders; one utterance carries the identity target, one a contour."""
    rng = np.random.default_rng(11)
    Fs = (5, 37, 40, 9)
    mels = [(rng.uniform(-7.0, -1.0, size=(80, F)) + 2.0 * np.sin(np.arange(F) / 5.0)[None, :]).astype(np.float32) for F in Fs]
    targets = [pkg.PitchTarget(factor=0.9), pkg.PitchTarget(hz=150.0, range=2.0), pkg.PitchTarget(), pkg.PitchTarget(factor=1.0, range=0.0)]
    contours = [None, pkg.ProsodyContour(cr.CONTOURS["ramp"]), None, None]
    o = pkg.F0Opts(threshold=0.0)
    voc.set_seed(3)
    one, one_stats = [], []
    for m, t, c in zip(mels, targets, contours):
        one.append(voc.infer_pitch_target(m, t, c, opts=o))
        one_stats.append(voc.last_f0())
    assert np.array_equal(one[2], voc.infer(mels[2])) and one_stats[2] == []
    fwd = voc.infer_batch_pitch_target(mels, targets, contours, opts=o)
    st_fwd = voc.last_f0()
    rev = voc.infer_batch_pitch_target(mels[::-1], targets[::-1], contours[::-1], opts=o)[::-1]
    st_rev = voc.last_f0()[::-1]
    assert len(st_fwd) == len(st_rev) == 4
    for u, F in enumerate(Fs):
        Fp = cr.frames(cr.CONTOURS["ramp"], F) if u == 1 else F
        assert one[u].shape == fwd[u].shape == rev[u].shape == (256 * (Fp - 1),), u
        assert np.array_equal(fwd[u], one[u]) and np.array_equal(rev[u], one[u]), u
        assert stats_bits(st_fwd[u]) == stats_bits(st_rev[u]) and st_fwd[u].n_frames == F
        if u != 2:
            assert stats_bits(st_fwd[u]) == stats_bits(one_stats[u][0]), u


def test_infer_pitch_target_is_the_composition_of_its_parts(pkg, mel40):
    """output_normalise = 0: infer_pitch_target(mel) against infer_linear(pitch_target_linear(mel_to_linear(mel))), held to the
    distance the pair infer(mel) / infer_linear(mel_to_linear(mel)) shows (the method of test_gpu_contour.py); ms[0] covers
    everything in front of the loop."""
    v = pkg.create_griffin_lim(iters=30, seed=5)
    try:
        v.set_opts(output_normalise=0)
        S = v.mel_to_linear(mel40)
        d_pair = float(np.abs(v.infer(mel40) - v.infer_linear(S)).max())
        o = pkg.F0Opts(threshold=0.0)
        for t, c in ((pkg.PitchTarget(factor=1.1, range=2.0), None), (pkg.PitchTarget(hz=170.0), pkg.ProsodyContour(cr.CONTOURS["ramp"]))):
            whole = v.infer_pitch_target(mel40, t, c, opts=o)
            st = v.last_f0()
            t_ms = v.last_timings()
            parts = v.infer_linear(v.pitch_target_linear(S, t, c, opts=o)[0])
            d = float(np.abs(whole - parts).max())
            print("composition: max |whole - parts| %.3e (the pair without a target: %.3e); stats %s" % (d, d_pair, st[0].astuple()))
            assert whole.shape == parts.shape and np.all(np.isfinite(whole)) and d <= d_pair, (d, d_pair)
            assert len(st) == 1 and st[0].n_frames == 40 and st[0].n_voiced == 40 and t_ms["mel_to_linear_ms"] > 0
    finally:
        v.close()


def test_tracker_from_a_mel_and_from_audio_is_the_stage_behind_their_front_ends(pkg, voc, mel40):
    """xdtts_griffinlim_f0 == mel_to_linear then f0_linear, xdtts_griffinlim_f0_audio == analyze then f0_linear, bit for bit."""
    a, b = voc.f0(mel40), voc.f0_linear(voc.mel_to_linear(mel40))
    assert all(np.array_equal(a[k], b[k]) for k in range(3)) and stats_bits(a[3]) == stats_bits(b[3]) and a[3].n_frames == 40
    y = pr.voiced_signal(n=256 * 20 + 100, f0=180.0)
    S, _ = voc.analyze(y, want_mel=False)
    a, b = voc.f0_audio(y), voc.f0_linear(S)
    assert a[0].shape == (21,) and all(np.array_equal(a[k], b[k]) for k in range(3)) and stats_bits(a[3]) == stats_bits(b[3])
    inner = a[2][4:-4]
    assert np.all(inner > 0) and np.all(np.abs(fr.cents(inner, 180.0)) <= 30.0 + 1200.0 * np.log2(1.03))  # tracking bound + the vibrato's reach


def test_synthesize_entries(pkg, voc, model):
    """synthesize(target=) and synthesize_batch(target=) on the synthetic weights of smoke(), 12 decoder steps: the mel is the
    plain entry's bits, last_f0 reports n_frames = 12, the audio is infer_pitch_target's on that mel, and the batch equals the
    single entry (batch_shape = 4)."""
    ids = np.array([108, 119, 11, 88, 113, 108, 120, 11, 116, 7], dtype=np.int64)
    opts = pkg.default_opts(fixed_steps=12, dropout_seed=5)
    o = pkg.F0Opts(threshold=0.0)
    t = pkg.PitchTarget(hz=150.0, range=0.5)
    voc.set_seed(3)
    mel0, _ = pkg.synthesize(model, voc, ids, opts=opts)
    mel1, audio = pkg.synthesize(model, voc, ids, opts=opts, target=t, f0_opts=o)
    st = voc.last_f0()
    assert mel0.shape == (80, 12) and np.array_equal(mel0, mel1) and len(st) == 1 and st[0].n_frames == 12
    want = voc.infer_pitch_target(mel0, t, opts=o)
    assert audio.shape == (256 * 11,) and np.array_equal(audio, want) and stats_bits(voc.last_f0()[0]) == stats_bits(st[0])
    groups = [[ids], [synth_ids(10, seed=2)]]
    bopts = pkg.default_opts(dropout_seed=5)
    ts = [t, pkg.PitchTarget(factor=1.1)]
    mels, audios = pkg.synthesize_batch(model, voc, groups, opts=bopts, fixed_steps=[[12], [12]], target=ts, f0_opts=o)
    stb = voc.last_f0()
    m_plain, _ = pkg.synthesize_batch(model, voc, groups, opts=bopts, fixed_steps=[[12], [12]])
    assert len(stb) == 2 and all(s.n_frames == 12 for s in stb)
    for u in range(2):
        assert np.array_equal(mels[u], m_plain[u]) and mels[u].shape == (80, 12), u
        assert np.array_equal(audios[u], voc.infer_pitch_target(mels[u], ts[u], opts=o)), u


# the distance between the medians of the two chains, measured on an MI355X (profiles/f0.txt: 161.66 Hz and 161.60 Hz), in Hz
END_TO_END_MEDIAN_DISTANCE_HZ = 0.063


def test_end_to_end_the_audio_lands_on_the_target(pkg, voc, orc):
    """The log-mel of the 140 Hz voice (the GPU's own analysis) -> infer_pitch_target at 160 Hz, 30 iterations ->
    xdtts_griffinlim_f0_audio on the returned audio.  Beside it the fp32 CPU oracle chain given the same ratios: the oracle's
    mel -> linear, the float32 restatement of the stage, the oracle's Griffin-Lim.  Both medians are estimated by f0_ref on the
    audio's fp64 STFT magnitude at threshold 0 (the signal is voiced throughout; the audio of the loop carries a cepstral peak of
    about 0.15, under the default voicing threshold -- gpu_f0_cases.end_to_end); either further than 2 % from 160 Hz fails
    outright, and their distance is held to twice the value measured on an MI355X (profiles/f0.txt)."""
    voc.set_seed(3)
    r = gc.end_to_end(pkg, voc, orc, 160.0)
    st, st_audio, m_gpu, m_cpu = r["stats"], r["stats_audio"], r["median_gpu"], r["median_cpu"]
    assert stats_bits(st) == stats_bits(r["stats_hook"]) and st.n_voiced >= 0.9 * 64
    print("end to end: source median %.2f Hz, base %.4f; audio median gpu %.2f Hz, cpu chain %.2f Hz, distance %.3f Hz; f0_audio on the device: median %.2f Hz, median strength %.3f" % (
        st.median_hz, st.base_ratio, m_gpu, m_cpu, abs(m_gpu - m_cpu), st_audio.median_hz, r["strength_audio"]))
    assert abs(m_gpu / 160.0 - 1.0) <= 0.02 and abs(m_cpu / 160.0 - 1.0) <= 0.02, (m_gpu, m_cpu)
    assert abs(st_audio.median_hz / 160.0 - 1.0) <= 0.02, st_audio.median_hz
    assert END_TO_END_MEDIAN_DISTANCE_HZ is not None, "the distance has not been measured yet"
    assert abs(m_gpu - m_cpu) <= 2.0 * END_TO_END_MEDIAN_DISTANCE_HZ, (m_gpu, m_cpu)
