"""GPU tests of prosody contours (rate, pitch and gain that vary inside an utterance; k_prosody_contour): the stage against the
fp64 restatement of its definition (tests/contour_ref.py), exact zeros and the identity, the ragged form against the single one,
the composition of the entries, and the property the feature exists for -- the F0 of each half of the audio follows that half's
pitch."""
import ctypes as C

import numpy as np
import pytest

import contour_ref as cr
import prosody_ref as pr
from conftest import synth_ids

pytestmark = pytest.mark.gpu

STEP = cr.CONTOURS["step"]


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)
    v.set_opts(batch_shape=4)  # the single call's split into workgroups: a batch's audio is the single call's bit for bit
    yield v
    v.close()


@pytest.fixture(scope="module")
def mel40():
    rng = np.random.default_rng(11)
    mel = (rng.uniform(-7.0, -1.0, size=(80, 40)) + 2.0 * np.sin(np.arange(40) / 5.0)[None, :]).astype(np.float32)
    mel.setflags(write=False)
    return mel


@pytest.mark.parametrize("F", [2, 3, 5, 37])
@pytest.mark.parametrize("name", list(cr.CONTOURS))
def test_contour_linear_matches_the_fp64_reference(pkg, voc, name, F):
    """F = 2, 3, 5, 37 x five contours: reaches F' = 2, a partial last workgroup and more than one workgroup; a ramp behind an
    unmodified span, steps in all three fields, one point away from both ends, a muted span under a rate ramp, and five points
    with the extreme rates, pitches and gains.  Input: log-uniform over nine e-folds with 5 % exact zeros.  Metric and bound are
    those of tests/test_gpu_prosody.py: max |x - ref64| / max(ref64, log_floor) <= 4 x d32 + 2e-5, d32 = the same metric of the
    float32 restatement (on the CPU 1.3e-4 .. 1.0e-3 for these cases, 0 .. 6e-8 for `mute`, which never leaves the copy branch).
    On an MI355X err(gpu) is 1.3e-4 .. 9.9e-4 beside d32 1.3e-4 .. 9.9e-4, and 0 .. 5.9e-8 for `mute`; the test prints both per case.
    First of all the two restatements must take the same branch (copy or transform) in every output frame."""
    points = cr.CONTOURS[name]
    S = pr.random_magnitude(F, seed=100 + F)
    ref, b64 = cr.contour(S, points)
    r32, b32 = cr.contour(S, points, dtype=np.float32)
    assert np.array_equal(b64, b32), (name, F)
    d32 = pr.rel_err(r32, ref)
    out = voc.contour_linear(S, pkg.ProsodyContour(points))
    assert out.shape == ref.shape == (513, cr.frames(points, F)) and out.dtype == np.float32 and np.all(np.isfinite(out))
    dg = pr.rel_err(out, ref)
    print("contour %s F=%d F'=%d (%d copied): err(gpu) %.3e  d32 %.3e" % (name, F, out.shape[1], int(b64.sum()), dg, d32))
    assert dg <= 4.0 * d32 + 2e-5, (dg, d32)
    # exact: zeros where the reference has them and nowhere else in the copied frames; finite and positive behind the transform
    assert np.array_equal(out[:, b64] == 0, ref[:, b64] == 0), (name, F)
    if name == "mute":
        assert b64.all() and (ref == 0).sum() > (S == 0).sum() and np.array_equal(out == 0, ref == 0)
    moved = out[:, ~b64]
    gain_zero = np.all(ref[:, ~b64] == 0, axis=0)  # (a transformed frame under gain 0: none in these cases)
    assert not gain_zero.any() and np.all(moved > 0)


def test_other_lifter_and_floor_follow_the_reference_too(pkg, voc):
    S = pr.random_magnitude(9, seed=77)
    for kw in (dict(lifter=255), dict(lifter=1), dict(log_floor=1e-3)):
        ref, b64 = cr.contour(S, STEP, **kw)
        r32, b32 = cr.contour(S, STEP, dtype=np.float32, **kw)
        fl = kw.get("log_floor", 1e-5)
        out = voc.contour_linear(S, pkg.ProsodyContour(STEP, **kw))
        dg, d32 = pr.rel_err(out, ref, fl), pr.rel_err(r32, ref, fl)
        print("contour step %s: err(gpu) %.3e  d32 %.3e" % (kw, dg, d32))
        assert np.array_equal(b64, b32) and out.shape == ref.shape and dg <= 4.0 * d32 + 2e-5, (kw, dg, d32)


def test_unit_contours_return_S_itself(pkg, voc):
    """rate = pitch = gain = 1 everywhere: the bits of S, one frame included; and a rate-1 contour whose first half is all ones
    leaves that half's frames as they are (the copy branch on whole unmodified spans)."""
    S = pr.random_magnitude(37, seed=5)
    ident = pkg.ProsodyContour(cr.IDENTITY)
    assert np.array_equal(voc.contour_linear(S, ident), S)
    assert np.array_equal(voc.contour_linear(S[:, :1], ident), S[:, :1])
    assert np.array_equal(voc.contour_linear(S[:, :2], pkg.ProsodyContour([(0.5, 1.0, 1.0, 1.0)])), S[:, :2])
    half = [(0.0, 1.0, 1.0, 1.0), (0.5, 1.0, 1.0, 1.0), (0.5, 1.0, 1.25, 0.5)]
    out = voc.contour_linear(S, pkg.ProsodyContour(half))
    assert out.shape == S.shape and np.array_equal(out[:, :18], S[:, :18]) and np.all(out[:, 18:] > 0)


FS = (2, 3, 5, 9, 37, 40)
MIX = ("step", "identity", "five", "ramp", "one", "mute")  # F' = 3, 3, 5, 8, 52, 30: 101 rows, a partial last workgroup, and every
# boundary but one inside a workgroup in either order


@pytest.fixture(scope="module")
def ragged(pkg):
    mags = [pr.random_magnitude(F, seed=300 + F) for F in FS]
    for a in mags:
        a.setflags(write=False)
    points = [cr.IDENTITY if n == "identity" else cr.CONTOURS[n] for n in MIX]
    return mags, [pkg.ProsodyContour(p) for p in points], points


def test_ragged_form_equals_the_single_entry(pkg, voc, ragged):
    """Six utterances, F = 2, 3, 5, 9, 37, 40, the five contours and the identity, in both orders: every output is
    contour_linear's for that utterance alone, bit for bit; the identity utterance comes back as it went in."""
    mags, cons, points = ragged
    singles = [voc.contour_linear(S, c) for S, c in zip(mags, cons)]
    fwd = voc.contour_linear_batch(mags, cons)
    rev = voc.contour_linear_batch(mags[::-1], cons[::-1])[::-1]
    t = voc.last_timings()
    for u, F in enumerate(FS):
        assert singles[u].shape == (513, cr.frames(points[u], F)) == (513, (3, 3, 5, 8, 52, 30)[u]), u
        for name, out in (("forward", fwd[u]), ("reversed", rev[u])):
            assert out.shape == singles[u].shape and np.array_equal(out, singles[u]), (u, name)
    assert np.array_equal(fwd[1], mags[1]) and t["mel_to_linear_ms"] > 0


def test_infer_contour_is_the_composition_of_its_parts(pkg, mel40):
    """output_normalise = 0: infer_contour(mel) == infer_linear(contour_linear(mel_to_linear(mel))), held to the distance the
    existing pair infer(mel) / infer_linear(mel_to_linear(mel)) shows in the same test (the method of
    test_infer_prosody_is_the_composition_of_its_parts)."""
    v = pkg.create_griffin_lim(iters=30, seed=5)
    try:
        v.set_opts(output_normalise=0)
        S = v.mel_to_linear(mel40)
        d_pair = float(np.abs(v.infer(mel40) - v.infer_linear(S)).max())
        for name in ("step", "ramp", "five"):
            c = pkg.ProsodyContour(cr.CONTOURS[name])
            whole = v.infer_contour(mel40, c)
            parts = v.infer_linear(v.contour_linear(S, c))
            assert whole.shape == parts.shape == (256 * (cr.frames(cr.CONTOURS[name], 40) - 1),)
            d = float(np.abs(whole - parts).max())
            print("composition %s: max |whole - parts| %.3e (the pair without a contour: %.3e)" % (name, d, d_pair))
            assert np.all(np.isfinite(whole)) and d <= d_pair, (name, d, d_pair)
        t = v.last_timings()
        assert t["mel_to_linear_ms"] > 0 and t["iterations_ms"] > 0
    finally:
        v.close()


@pytest.mark.parametrize("phase_init", [0, 1])
def test_batched_vocoder_equals_the_single_entry(pkg, voc, phase_init):
    """infer_batch(mels, contour=cs)[u] is infer_contour(mels[u], cs[u]) bit for bit with batch_shape = 4, in both orders, with
    the seeded phase and with SPSI (phase_init 1): 256 (F' - 1) samples each."""
    rng = np.random.default_rng(11)
    Fs = (5, 37, 40, 9)
    mels = [(rng.uniform(-7.0, -1.0, size=(80, F)) + 2.0 * np.sin(np.arange(F) / 5.0)[None, :]).astype(np.float32) for F in Fs]
    names = ("five", "step", "identity", "ramp")
    points = [cr.IDENTITY if n == "identity" else cr.CONTOURS[n] for n in names]
    cs = [pkg.ProsodyContour(p) for p in points]
    voc.set_phase_init(phase_init)
    try:
        voc.set_seed(3)
        one = [voc.infer_contour(m, c) for m, c in zip(mels, cs)]
        voc.set_seed(3)
        fwd = voc.infer_batch(mels, contour=cs)
        voc.set_seed(3)
        rev = voc.infer_batch(mels[::-1], contour=cs[::-1])[::-1]
        voc.set_seed(3)
        assert np.array_equal(one[2], voc.infer(mels[2]))  # the identity utterance: the plain entry's bits
    finally:
        voc.set_phase_init(0)
    for u, F in enumerate(Fs):
        d = max(float(np.abs(fwd[u] - one[u]).max()), float(np.abs(rev[u] - one[u]).max())) if fwd[u].shape == one[u].shape == rev[u].shape else -1.0
        print("phase_init %d utterance %d F=%d F'=%d: max |batch - single| %.3e" % (phase_init, u, F, cr.frames(points[u], F), d))
        assert one[u].shape == fwd[u].shape == rev[u].shape == (256 * (cr.frames(points[u], F) - 1),), u
        assert np.all(np.isfinite(one[u])) and np.abs(one[u]).max() > 0, u
        assert np.array_equal(fwd[u], one[u]) and np.array_equal(rev[u], one[u]), u


def test_identity_returns_the_bits_of_the_plain_entries(pkg, voc, model, mel40):
    ident = pkg.ProsodyContour(cr.IDENTITY)
    voc.set_seed(3)
    assert np.array_equal(voc.infer_contour(mel40, ident), voc.infer(mel40))
    ids = synth_ids(24, seed=2)
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    mel0, audio0 = pkg.synthesize(model, voc, ids, opts=opts)
    mel1, audio1 = pkg.synthesize(model, voc, ids, opts=opts, contour=ident)
    assert np.array_equal(mel0, mel1) and np.array_equal(audio0, audio1) and audio0.size == 256 * 39
    groups = [[synth_ids(10, seed=2), synth_ids(8, seed=3)], [synth_ids(12, seed=6)]]
    steps = [[12, 14], [20]]
    bopts = pkg.default_opts(dropout_seed=5)
    m0, a0 = pkg.synthesize_batch(model, voc, groups, opts=bopts, fixed_steps=steps)
    m1, a1 = pkg.synthesize_batch(model, voc, groups, opts=bopts, fixed_steps=steps, contour=[ident, ident])
    assert all(np.array_equal(a, b) for a, b in zip(m0, m1)) and all(np.array_equal(a, b) for a, b in zip(a0, a1))


def test_synthesize_with_a_contour_returns_tacotron2s_own_mel(pkg, voc, model):
    ids = synth_ids(24, seed=2)
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    mel0, _ = pkg.synthesize(model, voc, ids, opts=opts)
    mel1, audio = pkg.synthesize(model, voc, ids, opts=opts, contour=pkg.ProsodyContour(STEP))
    Fp = cr.frames(STEP, 40)
    assert mel0.shape == (80, 40) and np.array_equal(mel0, mel1)
    assert Fp == pkg.prosody_contour_frames(pkg.ProsodyContour(STEP), 40) and Fp != 40
    assert audio.shape == (256 * (Fp - 1),) and np.all(np.isfinite(audio)) and np.abs(audio).max() > 0
    voc.set_seed(3)
    assert np.array_equal(audio, voc.infer_contour(mel0, pkg.ProsodyContour(STEP)))


def test_synthesize_batch_equals_its_two_halves(pkg, voc, model):
    """synthesize_batch(contour=cs) == tacotron2.infer_batch, the chunk mels of an utterance side by side, then
    infer_batch(mels, contour=cs), bit for bit; the mels returned are the unmodified ones."""
    groups = [[synth_ids(10, seed=2), synth_ids(8, seed=3)], [synth_ids(9, seed=4), synth_ids(11, seed=5)], [synth_ids(12, seed=6)]]
    steps = [[12, 14], [16, 18], [20]]
    points = [STEP, cr.IDENTITY, cr.CONTOURS["ramp"]]
    cs = [pkg.ProsodyContour(p) for p in points]
    opts = pkg.default_opts(dropout_seed=5)
    chunk_mels = model.infer_batch([c for g in groups for c in g], opts=opts, fixed_steps=[s for g in steps for s in g])
    want_mels = [np.concatenate(chunk_mels[0:2], axis=1), np.concatenate(chunk_mels[2:4], axis=1), chunk_mels[4]]
    voc.set_seed(3)
    want_audio = voc.infer_batch(want_mels, contour=cs)
    voc.set_seed(3)
    mels, audios = pkg.synthesize_batch(model, voc, groups, opts=opts, fixed_steps=steps, contour=cs)
    for u, F in enumerate((26, 34, 20)):
        assert mels[u].shape == (80, F) and np.array_equal(mels[u], want_mels[u]), u
        assert audios[u].shape == (256 * (cr.frames(points[u], F) - 1),) and np.array_equal(audios[u], want_audio[u]), u


# ---- the property the feature exists for ----------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def voiced96(voc):
    """The voiced signal (256 * 95 samples), its magnitude (513, 96) from the GPU's own analysis, and the F0 of the two windows
    of the identity run (30 iterations)."""
    y = pr.voiced_signal(256 * 95)
    S, _ = voc.analyze(y, want_mel=False)
    S.setflags(write=False)
    voc.set_seed(3)
    return S, halves_f0(voc.infer_linear(S, iters=30))


def halves_f0(audio):
    n = audio.size
    return pr.f0_autocorr(audio[n // 12 : 5 * n // 12]), pr.f0_autocorr(audio[7 * n // 12 : 11 * n // 12])


@pytest.mark.parametrize("first, second", [(1.0, 1.25), (0.8, 1.25)])
def test_f0_follows_the_pitch_of_each_half(pkg, voc, voiced96, first, second):
    """The voiced signal's own magnitude (F = 96) -> a rate-1 contour with a pitch step at pos 0.5 -> 30 iterations.  F0 over
    samples [n/12, 5n/12] and [7n/12, 11n/12], each divided by the identity run's F0 over the same window, must be within 4 %
    of that half's pitch (the bound of test_f0_follows_pitch_and_ignores_rate).  A numpy Griffin-Lim prototype (fp64, another
    phase seed) gave 1.0000 / 1.2496 and 0.8001 / 1.2496.  The same chain through the fp32 CPU oracle's Griffin-Lim in place of
    the GPU's (contour_ref in float32 on the fp64 magnitude, the oracle's seeded phase) gives 1.0000 / 1.2502 and 0.8002 / 1.2502.  The test prints the GPU's ratios (MI355X: 1.0000 / 1.2502 and 0.8002 / 1.2502)."""
    S, f0_ident = voiced96
    points = [(0.0, 1.0, first, 1.0), (0.5, 1.0, first, 1.0), (0.5, 1.0, second, 1.0)]
    voc.set_seed(3)
    audio = voc.infer_linear(voc.contour_linear(S, pkg.ProsodyContour(points)), iters=30)
    assert audio.size == 256 * 95 and np.all(np.isfinite(audio))
    f0 = halves_f0(audio)
    ratios = (f0[0] / f0_ident[0], f0[1] / f0_ident[1])
    print("pitch %g -> %g: F0 %.1f / %.1f Hz, identity %.1f / %.1f Hz, ratios %.4f / %.4f" % (first, second, f0[0], f0[1], f0_ident[0], f0_ident[1], *ratios))
    assert abs(ratios[0] / first - 1.0) <= 0.04 and abs(ratios[1] / second - 1.0) <= 0.04, ratios


def test_bad_fields_are_rejected_on_a_live_handle(pkg, voc, mel40):
    S = np.ones((513, 3), dtype=np.float32)
    bad = ([(0.0, 0.2, 1.0, 1.0)], [(0.0, 1.0, 2.5, 1.0)], [(0.0, 1.0, 1.0, 9.0)], [(0.6, 2.0, 1.0, 1.0), (0.5, 2.0, 1.0, 1.0)], [(1.5, 2.0, 1.0, 1.0)], [])
    for points in bad:
        for call in (lambda c: voc.contour_linear(S, c), lambda c: voc.infer_contour(mel40, c), lambda c: voc.infer_batch([mel40], contour=[c]),
                     lambda c: voc.contour_linear_batch([S, S], [pkg.ProsodyContour(STEP), c])):
            with pytest.raises(pkg.XdttsError) as e:
                call(pkg.ProsodyContour(points))
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    for kw in (dict(lifter=0), dict(log_floor=0.0)):
        with pytest.raises(pkg.XdttsError) as e:
            voc.contour_linear(S, pkg.ProsodyContour(STEP, **kw))
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    with pytest.raises(pkg.XdttsError) as e:  # one frame, and not the identity
        voc.contour_linear(S[:, :1], pkg.ProsodyContour(STEP))
    assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    out, nf = np.zeros((513, 16), dtype=np.float32), C.c_size_t(7)
    st = pkg.lib.xdtts_griffinlim_contour_linear(voc._h, None, 3, C.byref(pkg.ProsodyContour(STEP)), out.ctypes.data_as(C.c_void_p), C.byref(nf))
    assert st == pkg.XDTTS_ERR_BAD_ARG and nf.value == 0
    # and the handle still works
    assert np.array_equal(voc.contour_linear(S, pkg.ProsodyContour(cr.IDENTITY)), S)
    ref, _ = cr.contour(S, STEP)
    assert voc.contour_linear(S, pkg.ProsodyContour(STEP)).shape == ref.shape
