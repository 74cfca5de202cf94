"""GPU tests of the timbre stage (vocal-tract length and breathiness on the magnitude behind the prosody stage and in front of
the initial phase): k_timbre against the fp64 restatement of its definition (tests/timbre_ref.py), the identity, the ragged
launch against the single one bit for bit, the composition of the entries that honour the handle's setting, the sequence and
document entries, the three properties the stage exists for on the device's own output, the F0 of the audio, argument errors."""
import ctypes as C
import functools

import numpy as np
import pytest

import prosody_ref as pr
import timbre_ref as tr
from conftest import synth_ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)
    yield v
    v.close()


@functools.lru_cache(maxsize=None)
def _case(F, vtl, breath, lifter=30, log_floor=1e-5):
    """(input, fp64 reference, d32): computed once, shared, never written to"""
    S = tr.random_magnitude(F, seed=200 + F)
    ref = tr.timbre(S, vtl=vtl, breath=breath, seed=9, lifter=lifter, log_floor=log_floor)
    d32 = tr.rel_err(tr.timbre(S, vtl=vtl, breath=breath, seed=9, lifter=lifter, log_floor=log_floor, dtype=np.float32), ref, log_floor)
    for a in (S, ref):
        a.setflags(write=False)
    return S, ref, d32


def _mel(F, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 2.0 * np.sin(np.arange(F) / 5.0)[None, :]).astype(np.float32)


# ---- 1. the stage against the fp64 reference -----------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 3, 5, 37])
@pytest.mark.parametrize("vtl, breath", tr.CASES)
def test_timbre_linear_matches_the_fp64_reference(pkg, voc, F, vtl, breath):
    """F = 1, 3, 5, 37 x (vtl, breath): one row, a partial workgroup, more than one workgroup, many workgroups with a ragged
    tail; the envelope warp alone (non-dyadic and dyadic, positions beyond Nyquist for vtl > 1), the noise alone, both.  Input:
    log-uniform over nine e-folds with 5 % exact zeros.  Metric and rule are the prosody test's own: max |x - ref64| /
    max(ref64, log_floor) <= 4 x d32 + 2e-5, d32 = the same metric of the float32 restatement.  Every cell is finite and > 0
    (the floor enters the logarithm).  The test prints err(gpu) and d32 of every case; profiles/timbre.txt records them."""
    S, ref, d32 = _case(F, vtl, breath)
    out = voc.timbre_linear(S, pkg.Timbre(vtl=vtl, breath=breath, seed=9))
    assert out.shape == ref.shape == (513, F) and out.dtype == np.float32
    assert np.all(np.isfinite(out)) and np.all(out > 0)
    dg = tr.rel_err(out, ref)
    print("timbre F=%d vtl=%g breath=%g: err(gpu) %.3e  d32 %.3e" % (F, vtl, breath, dg, d32))
    assert dg <= 4.0 * d32 + 2e-5, (dg, d32)


@pytest.mark.parametrize("kw", [dict(lifter=1), dict(lifter=255), dict(log_floor=1e-3)], ids=["lifter1", "lifter255", "floor1e-3"])
def test_other_lifter_and_floor_follow_the_reference_too(pkg, voc, kw):
    """The two remaining fields away from their defaults at F = 9, same rule."""
    S, ref, d32 = _case(9, 0.7, 0.4, **kw)
    out = voc.timbre_linear(S, pkg.Timbre(vtl=0.7, breath=0.4, seed=9, **kw))
    dg = tr.rel_err(out, ref, kw.get("log_floor", 1e-5))
    print("timbre %s: err(gpu) %.3e  d32 %.3e" % (kw, dg, d32))
    assert out.shape == ref.shape and np.all(np.isfinite(out)) and np.all(out > 0)
    assert dg <= 4.0 * d32 + 2e-5, (kw, dg, d32)


# ---- 2. the identity ----------------------------------------------------------------------------------------------------------

def test_identity_returns_the_bits_of_the_plain_entries(pkg, voc, model):
    ident = pkg.Timbre()
    assert (ident.vtl, ident.breath) == (1.0, 0.0)
    assert voc.get_timbre().astuple() == ident.astuple()  # a fresh handle holds the default
    S = pr.random_magnitude(37, seed=5)
    assert np.array_equal(voc.timbre_linear(S, ident), S)
    assert np.array_equal(voc.timbre_linear(S[:, :1], ident), S[:, :1])
    assert np.array_equal(voc.timbre_linear(S, pkg.Timbre(seed=77, lifter=3, log_floor=0.5)), S)  # vtl and breath alone decide
    mel = _mel(40)
    p = pkg.Prosody(rate=1.25, pitch=0.8)
    ids = synth_ids(24, seed=2)
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)

    def run():
        voc.set_seed(3)
        return [voc.infer(mel), voc.infer_prosody(mel, p), voc.infer_batch([mel, mel[:, :12]])[1]] + list(pkg.synthesize(model, voc, ids, opts=opts))

    fresh = run()
    voc.set_timbre(ident)
    assert voc.get_timbre().astuple() == ident.astuple()
    for a, b in zip(fresh, run()):
        assert np.array_equal(a, b)
    voc.set_timbre(pkg.Timbre(vtl=1.25, breath=0.3, seed=4))
    assert voc.get_timbre().astuple() == (1.25, float(np.float32(0.3)), 4, 30, float(np.float32(1e-5)))
    changed = run()
    assert changed[0].shape == fresh[0].shape and not np.array_equal(changed[0], fresh[0])
    assert np.array_equal(changed[3], fresh[3])  # the mel is Tacotron2's own
    voc.set_timbre(None)  # NULL = the default: off again
    assert voc.get_timbre().astuple() == ident.astuple()
    for a, b in zip(fresh, run()):
        assert np.array_equal(a, b)


# ---- 3. batch == single, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (3, 0, 4, 2, 1)])
def test_ragged_launch_equals_the_single_launch(pkg, voc, order):
    """F = [1, 5, 2, 37, 4] under the identity, two seeds, vtl alone, breath alone and both, in two orders: every S_outs[u] is
    timbre_linear of that utterance alone -- the noise follows the frame inside its own utterance, not the row of the batch."""
    Fs = [1, 5, 2, 37, 4]
    ts = [pkg.Timbre(), pkg.Timbre(vtl=0.8, breath=0.5, seed=1), pkg.Timbre(vtl=1.6), pkg.Timbre(breath=1.0, seed=2), pkg.Timbre(vtl=0.5, breath=0.25, seed=2)]
    Ss = [pr.random_magnitude(F, seed=40 + u) for u, F in enumerate(Fs)]
    single = [voc.timbre_linear(S, t) for S, t in zip(Ss, ts)]
    assert np.array_equal(single[0], Ss[0])
    outs = voc.timbre_linear_batch([Ss[u] for u in order], [ts[u] for u in order])
    for k, u in enumerate(order):
        assert outs[k].shape == (513, Fs[u]) and np.array_equal(outs[k], single[u]), (order, u)
    # a batch of identities alone touches nothing and returns the inputs' bits
    same = voc.timbre_linear_batch(Ss[:3], [pkg.Timbre()] * 3)
    assert all(np.array_equal(a, b) for a, b in zip(same, Ss))


# ---- 4. composition -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase_init", [0, 1])
def test_infer_under_a_timbre_is_the_composition_of_its_parts(pkg, phase_init):
    """output_normalise = 0, a 40-frame mel, a timbre set: infer(mel) == infer_linear(timbre_linear(mel_to_linear(mel))) and
    infer_prosody(mel, p) == infer_linear(timbre_linear(prosody_linear(mel_to_linear(mel), p))), each held to the distance the
    plain pair infer / infer_linear shows here with the setting off (the rule of test_infer_prosody_is_the_composition_of_its_parts).
    phase_init 1: SPSI runs on S'.  Then infer_batch of three mels (F = 5, 40, 12, batch_shape 4) under the setting against the
    single calls, held to the degree infer_batch agrees with infer with the setting off, measured here."""
    mel = _mel(40)
    t = pkg.Timbre(vtl=1.25, breath=0.3, seed=4)
    v = pkg.create_griffin_lim(iters=30, seed=5)
    try:
        v.set_opts(output_normalise=0, batch_shape=4)
        v.set_phase_init(phase_init)
        S = v.mel_to_linear(mel)
        d_pair = float(np.abs(v.infer(mel) - v.infer_linear(S)).max())
        mels = [mel[:, :5], mel, mel[:, 20:32]]
        off_single = [v.infer(m) for m in mels]
        d_batch_off = max(float(np.abs(a - b).max()) for a, b in zip(v.infer_batch(mels), off_single))
        v.set_timbre(t)
        St = v.timbre_linear(S, t)
        whole, parts = v.infer(mel), v.infer_linear(St)
        d = float(np.abs(whole - parts).max())
        print("composition phase_init %d: max |infer - parts| %.3e (the pair without timbre: %.3e)" % (phase_init, d, d_pair))
        assert whole.shape == parts.shape == (256 * 39,) and d <= d_pair, (d, d_pair)
        ms = v.last_timings()
        assert ms["mel_to_linear_ms"] > 0 and ms["iterations_ms"] > 0
        for kw in (dict(rate=1.25), dict(rate=0.7, pitch=1.3)):
            p = pkg.Prosody(**kw)
            whole = v.infer_prosody(mel, p)
            parts = v.infer_linear(v.timbre_linear(v.prosody_linear(S, p), t))
            d = float(np.abs(whole - parts).max())
            print("composition phase_init %d %s: max |infer_prosody - parts| %.3e (pair: %.3e)" % (phase_init, kw, d, d_pair))
            assert whole.shape == parts.shape == (256 * (pkg.prosody_frames(40, p.rate) - 1),) and d <= d_pair, (kw, d, d_pair)
        # infer_linear itself does not honour the setting
        assert np.array_equal(v.infer_linear(S), v.infer_linear(S)) and not np.array_equal(v.infer_linear(S), v.infer(mel))
        on_single = [v.infer(m) for m in mels]
        d_batch_on = max(float(np.abs(a - b).max()) for a, b in zip(v.infer_batch(mels), on_single))
        print("batch phase_init %d: max |infer_batch - infer| %.3e under the timbre, %.3e without" % (phase_init, d_batch_on, d_batch_off))
        assert d_batch_on <= d_batch_off, (d_batch_on, d_batch_off)
        assert all(not np.array_equal(a, b) for a, b in zip(on_single, off_single))
    finally:
        v.close()


# ---- 5. through the model -----------------------------------------------------------------------------------------------------

def test_sequence_and_document_under_a_timbre(pkg, voc, model):
    """synthesize_sequence of two 24-id utterances under a timbre == two synthesize calls under it, bit for bit (the sequence
    entry's guarantee); the mels are those of the run without timbre; synthesize_document of the same two as fp32 at level 0 ==
    xdtts_griffinlim_join of the two audios."""
    ids = [synth_ids(24, seed=2), synth_ids(24, seed=3)]
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    voc.set_seed(3)
    voc.set_timbre(None)
    plain = [pkg.synthesize(model, voc, x, opts=opts) for x in ids]
    try:
        voc.set_timbre(pkg.Timbre(vtl=0.8, breath=0.5, seed=6))
        single = [pkg.synthesize(model, voc, x, opts=opts) for x in ids]
        mels, audios = pkg.synthesize_sequence(model, voc, ids, opts=opts)
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
        voc.set_timbre(None)


# ---- 6. the properties, on the device's stage output --------------------------------------------------------------------------

def test_properties_on_the_device(pkg, voc):
    """The three conditions of the CPU test with the same inputs and bounds, on timbre_linear's output: the period under vtl,
    the cepstral-peak ratios under breath, the bump's power centroid."""
    lines = []
    tr.check_properties(lambda S, vtl, breath: voc.timbre_linear(S, pkg.Timbre(vtl=vtl, breath=breath)), say=lines.append)
    print("timbre on the device: " + "; ".join(lines))


# ---- 7. F0 stays in the audio -------------------------------------------------------------------------------------------------

def test_f0_stays_in_the_audio(pkg, voc):
    """The voiced signal's own magnitude (voc.analyze) -> timbre_linear at vtl 0.8 and 1.25 -> 30 iterations: the F0 of the
    middle half over the identity run's F0 is within 4 % of 1 (the bound test_f0_follows_pitch_and_ignores_rate uses for this
    chain).  The same chain from the fp64 reference's magnitude is run beside it and printed."""
    y = pr.voiced_signal(256 * 47)
    S, _ = voc.analyze(y)

    def f0_of(mag):
        voc.set_seed(3)
        audio = voc.infer_linear(np.ascontiguousarray(mag, dtype=np.float32), iters=30)
        assert audio.size == 256 * 47 and np.all(np.isfinite(audio))
        return pr.f0_autocorr(audio[audio.size // 4 : 3 * audio.size // 4])

    f_id = f0_of(S)
    for vtl in (0.8, 1.25):
        f_dev = f0_of(voc.timbre_linear(S, pkg.Timbre(vtl=vtl)))
        f_ref = f0_of(tr.timbre(S, vtl=vtl))
        print("F0 under vtl %g: device %.1f Hz (ratio %.4f), fp64 reference's magnitude %.1f Hz (ratio %.4f), identity %.1f Hz" %
              (vtl, f_dev, f_dev / f_id, f_ref, f_ref / f_id, f_id))
        assert abs(f_dev / f_id - 1.0) <= 0.04, (vtl, f_dev, f_id, f_ref)


# ---- 8. argument errors -------------------------------------------------------------------------------------------------------

def test_bad_fields_are_rejected_on_a_live_handle(pkg, voc):
    S = np.ones((513, 3), dtype=np.float32)
    keep = pkg.Timbre(vtl=1.5, breath=0.25, seed=8, lifter=40, log_floor=1e-4)
    voc.set_timbre(keep)
    try:
        for field, v in (("vtl", 0.49), ("vtl", 2.5), ("vtl", float("nan")), ("breath", -0.1), ("breath", 1.5), ("breath", float("inf")),
                         ("lifter", 0), ("lifter", 256), ("log_floor", 0.0), ("log_floor", float("nan"))):
            bad = pkg.Timbre(**{field: v})
            for call in (lambda: voc.set_timbre(bad), lambda: voc.timbre_linear(S, bad)):
                with pytest.raises(pkg.XdttsError) as e:
                    call()
                assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and field in str(e.value), (field, v, str(e.value))
            assert voc.get_timbre().astuple() == keep.astuple()  # a failed set leaves the setting as it was
        with pytest.raises(pkg.XdttsError) as e:
            voc.timbre_linear_batch([S, S, S], [pkg.Timbre(), pkg.Timbre(vtl=3.0), pkg.Timbre()])
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and "utterance 1" in str(e.value) and "vtl" in str(e.value)
        out = np.zeros((513, 3), dtype=np.float32)
        good = pkg.Timbre(vtl=1.25)
        assert pkg.lib.xdtts_griffinlim_timbre_linear(voc._h, None, 3, C.byref(good), out.ctypes.data_as(C.c_void_p)) == pkg.XDTTS_ERR_BAD_ARG
        assert pkg.lib.xdtts_griffinlim_timbre_linear(voc._h, S.ctypes.data_as(C.c_void_p), 0, C.byref(good), out.ctypes.data_as(C.c_void_p)) == pkg.XDTTS_ERR_BAD_ARG
        # and the handle still works: one frame is enough for the stage
        one = voc.timbre_linear(S[:, :1], good)
        assert one.shape == (513, 1) and np.all(np.isfinite(one)) and np.all(one > 0)
    finally:
        voc.set_timbre(None)
