"""GPU parity of the vocoder at every engine and work split its frame count can select (tests/gl_shapes.py
restates the rules; test_gl_shapes_cpu.py shows that these frame counts reach every class on 256 CUs):
the two-kernel path at its last sizes, k_gl_persistent<4> with 3-frame workgroups, k_gl_persistent<8>
launched with 5, 6, 7 and 8 waves, the launch-per-iteration k_gl_fused, the batch shapes with their segment
table, the step hook's state export and the phase drawn in the kernel -- each against the fp64 oracle.

Four iterations from a fixed phase keep fp32 rounding noise small: the fp32 oracle against the fp64 oracle
on this input shows a whole-signal RMS of 1.8e-7 .. 1.8e-6 and a worst hop of 3.4e-7 .. 5.7e-5 (F = 2049).
The conditions:
  whole-signal RMS against fp64   <= 2 x the fp32 oracle's + 1e-6   (the suite's rule for free-running audio)
  RMS against the fp32 oracle     <= 1e-4                           (the suite's bar)
  worst hop against fp64          <= 1e-3
The last one is 17 x the largest figure the reference alone shows and about 100 x below what one missing or
doubled frame contribution gives in a hop (signal RMS 0.23, one of four overlapping frames 0.05 .. 0.1), and,
unlike the whole-signal RMS, it does not shrink with the length of the utterance.
Every test prints its figures ("gl-shapes ..." lines: pytest -rA shows them for passing tests too)."""
import os
import sys

import numpy as np
import pytest

import gl_shapes as gs
from gl_shapes import rms

pytestmark = pytest.mark.gpu
ITERS = 4
SEED = 3
HOP_BOUND = 1e-3
FRAME_BOUND = 1e-4
TIMED_OUT = "exchange timed out"


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=ITERS, seed=SEED)
    yield v
    v.close()


class forced_env:
    """Sets one of the library's per-call environment switches and restores the previous state."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def assert_no_fallback(capfd):
    """The persistent engine did not quietly hand the case to the fallback; what the test printed is handed back
    to pytest's capture so that the figures stay in the report."""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    sys.stderr.write(cap.err)
    assert TIMED_OUT not in cap.err, cap.err


_AUDIO_REF = {}


def audio_ref(orc, orc64, F):
    """S, phase0 and the two oracles' audio after ITERS iterations: computed once per F, never modified."""
    if F not in _AUDIO_REF:
        S = gs.chirp_S(orc, F)
        p0 = orc.phase_init(SEED, gs.N_BINS, F)
        f32 = orc.griffinlim(S, phase0=p0, iters=ITERS)
        f64 = orc64.griffinlim(S, phase0=p0, iters=ITERS)
        for a in (S, p0, f32, f64):
            a.setflags(write=False)
        _AUDIO_REF[F] = (S, p0, f32, f64)
    return _AUDIO_REF[F]


def check_audio(tag, F, a, f32, f64):
    """The four assertions of the module docstring; prints the figures first."""
    assert a.shape == (gs.HOP * (F - 1),) and a.dtype == np.float32, (tag, F, a.shape)
    assert np.all(np.isfinite(a)), (tag, F)
    eg, ef, e32 = rms(a, f64), rms(f32, f64), rms(a, f32)
    hg, hf = gs.worst_hop(a, f64), gs.worst_hop(f32, f64)
    print("gl-shapes %-16s F=%5d %-16s rms gpu-f64 %.2e  f32-f64 %.2e  gpu-f32 %.2e  worst hop gpu-f64 %.2e (hop %d)  f32-f64 %.2e" % (
        tag, F, gs.shape_class(F), eg, ef, e32, hg, int(np.argmax(gs.hop_rms(a, f64))), hf), flush=True)
    assert eg <= 2.0 * ef + 1e-6, (tag, F, eg, ef)
    assert e32 <= 1e-4, (tag, F, e32)
    assert hg <= HOP_BOUND, (tag, F, hg, int(np.argmax(gs.hop_rms(a, f64))))
    return eg, hg


@pytest.mark.parametrize("F", gs.SWEEP_DEFAULT)
def test_sweep_default_engine(voc, orc, orc64, capfd, F):
    """(a) infer_linear on the engine the frame count selects.  MI355X, against fp64 (the fp32 oracle's own figure in brackets):
        F     class            whole-signal rms       worst hop
        10    tiny             1.6e-7 (2.4e-7)        2.6e-7 (4.6e-7)
        15    tiny             3.5e-6 (1.7e-6)        1.0e-5 (4.9e-6)
        16    p4 all 4         1.4e-6 (1.8e-6)        4.8e-6 (6.0e-6)
        17    p4 3s inside     1.6e-7 (1.8e-7)        3.1e-7 (3.4e-7)
        18    p4 3s inside     2.5e-7 (2.2e-7)        6.2e-7 (4.9e-7)
        19    p4 3 first       2.9e-7 (3.2e-7)        5.7e-7 (6.6e-7)
        21    p4 3s inside     1.6e-7 (2.8e-7)        2.4e-7 (5.9e-7)
        37    p4 3s inside     1.6e-7 (2.2e-7)        3.7e-7 (5.4e-7)
        203   p4 3 first       2.7e-7 (3.2e-7)        1.5e-6 (2.0e-6)
        1024  p4 all 4         3.2e-7 (3.2e-7)        3.4e-6 (2.8e-6)
        1026  p8 TF 5          3.0e-7 (3.4e-7)        2.8e-6 (4.7e-6)
        1281  p8 TF 6          2.3e-7 (2.9e-7)        1.5e-6 (3.8e-6)
        1537  p8 TF 7          2.4e-7 (2.9e-7)        2.3e-6 (3.5e-6)
        1793  p8 TF 8 mixed    2.5e-7 (2.6e-7)        1.8e-6 (2.2e-6)
        2048  p8 TF 8 even     9.5e-7 (9.8e-7)        2.6e-5 (2.9e-5)
        2049  launch           2.5e-6 (1.3e-6)        1.1e-4 (5.7e-5), hop 2047 for both
    F = 1026 FAILED when this test was written (worst hop 4.65e-2 at hop 0, whole-signal rms 1.6e-3): launches of 5, 6 and
    7 waves took every sample's window sum at the thread's first offset in the hop, which is wrong in the first and last
    three hops of the utterance; fixed in k_gl_persistent with this test."""
    S, p0, f32, f64 = audio_ref(orc, orc64, F)
    with forced_env("XDTTS_GL", None):
        a = voc.infer_linear(S, phase0=p0, iters=ITERS)
    check_audio("default", F, a, f32, f64)
    assert_no_fallback(capfd)


@pytest.mark.parametrize("F", gs.SWEEP_LAUNCH)
def test_sweep_launch_engine(voc, orc, orc64, capfd, F):
    """(b) the same with XDTTS_GL=launch (read on every call): k_gl_fused<4> with ping-pong angles under graph
    replay, the engine of every demoted handle and of every utterance above 2048 frames; and the two engines
    agree within 1e-4 RMS at the same F.  MI355X: whole-signal rms against fp64 2.4e-7 .. 1.6e-6 below 2049 and 2.5e-6
    there, worst hop 4.5e-7 .. 5.4e-6 below 2049 and 1.1e-4 there; the two engines 2.2e-7 .. 3.0e-6 apart."""
    S, p0, f32, f64 = audio_ref(orc, orc64, F)
    with forced_env("XDTTS_GL", "launch"):
        b = voc.infer_linear(S, phase0=p0, iters=ITERS)
    with forced_env("XDTTS_GL", None):
        a = voc.infer_linear(S, phase0=p0, iters=ITERS)
    check_audio("launch", F, b, f32, f64)
    e = rms(a, b)
    print("gl-shapes launch           F=%5d default-vs-launch rms %.2e" % (F, e), flush=True)
    assert e <= 1e-4, (F, e)
    assert_no_fallback(capfd)


_STEP_REF = {}


def step_ref(orc, orc64, F):
    """The two start states and, for each, both oracles' state after two more iterations."""
    if F not in _STEP_REF:
        S, p0 = audio_ref(orc, orc64, F)[:2]
        zero = np.zeros_like(p0)
        starts = [(p0, zero), orc.griffinlim_step(S, p0, zero, iters=3)]  # (the second: momentum term live)
        out = []
        for a, r in starts:
            o32 = orc.griffinlim_step(S, a, r, iters=2)
            o64 = orc64.griffinlim_step(S, a, r, iters=2)
            for x in (a, r) + tuple(o32) + tuple(o64):
                x.setflags(write=False)
            out.append((a, r, o32, o64))
        _STEP_REF[F] = out
    return _STEP_REF[F]


@pytest.mark.parametrize("engine", ["default", "launch"])
@pytest.mark.parametrize("F", gs.SWEEP_STEP)
def test_step_hook(voc, orc, orc64, capfd, F, engine):
    """(c) xdtts_griffinlim_step, two iterations from (phase0, 0) and from the fp32 oracle's state after three:
    on the persistent engine the final state leaves through ang_out / tprev_out, indexed by fbase + f.  The
    rebuilt spectrum is held per frame (a mis-indexed row is O(1) in its frame, and 1 / sqrt(F) overall).  MI355X, worst
    of the 14 cases of each engine: rebuilt spectrum overall 1.5e-6 (default, F = 16) / 5.8e-7 (launch), per frame 6.0e-6
    (default, F = 1026, frame 169; the fp32 oracle 7.3e-6 there) / 5.2e-6 (launch), angles 1.9e-5 / 2.9e-5 (launch, F = 17,
    second state: the fp32 oracle 1.5e-5, so the rule allows 3.1e-5)."""
    S = audio_ref(orc, orc64, F)[0]
    for i, (a, r, (oa, orr), (da, dr)) in enumerate(step_ref(orc, orc64, F)):
        with forced_env("XDTTS_GL", "launch" if engine == "launch" else None):
            ga, gr = voc.step(S, a, r, n_iter=2)
        assert ga.shape == gr.shape == (gs.N_BINS, F, 2) and np.all(np.isfinite(ga)) and np.all(np.isfinite(gr))
        sig = float(np.sqrt(np.mean(dr ** 2)))
        eg, ef = rms(gr, dr) / sig, rms(orr, dr) / sig
        pg, pf = gs.per_frame_rel(gr, dr), gs.per_frame_rel(orr, dr)
        ag, af = rms(ga, da), rms(oa, da)
        print("gl-shapes step/%-7s F=%5d state %d  rebuilt rel gpu-f64 %.2e  f32-f64 %.2e  per frame gpu-f64 %.2e (frame %d)  f32-f64 %.2e  "
              "angles gpu-f64 %.2e  f32-f64 %.2e" % (engine, F, i, eg, ef, pg.max(), int(np.argmax(pg)), pf.max(), ag, af), flush=True)
        assert eg <= 2.0 * ef + 1e-6, (F, engine, i, eg, ef)
        assert pg.max() <= FRAME_BOUND, (F, engine, i, float(pg.max()), int(np.argmax(pg)))
        assert ag <= 2.0 * af + 1e-6, (F, engine, i, ag, af)
    assert_no_fallback(capfd)


_BATCH_REF = {}


def batch_ref(orc, orc64, seed):
    """Per utterance of the batch: the mel, and both oracles' audio from the oracle's own mel -> linear."""
    if seed not in _BATCH_REF:
        pinv = orc.pinv(orc.mel_filter_bank())
        out = []
        for u, F in enumerate(gs.BATCH_FRAMES):
            mel = gs.speech_mel(F, 100 + u)
            S = orc.mel_to_linear(pinv, mel, power=1.7)
            f32 = orc.griffinlim(S, seed=seed, iters=ITERS)
            f64 = orc64.griffinlim(S, seed=seed, iters=ITERS)
            for x in (mel, f32, f64):
                x.setflags(write=False)
            out.append((F, mel, f32, f64))
        _BATCH_REF[seed] = out
    return _BATCH_REF[seed]


@pytest.mark.parametrize("form", ["shape4", "force42", "force8"])
def test_batch_against_the_reference(pkg, orc, orc64, capfd, form):
    """(d) one infer_batch of F = 16, 17, 19, 37, 64, 203, 5 (the last one on the two-kernel path), forward and
    reversed so that every abase / fbase is non-trivial, each utterance against the fp64 oracle of ITS mel:
    k_gl_persistent<4> or <4, 2> (batch_shape = 4), <4, 2> forced, and <8> with 5 .. 8 own frames.  MI355X, worst of
    the 14 audios of each form: whole-signal rms 3.2e-7 / 3.2e-7 / 5.3e-7 (at most 0.22 / 0.22 / 0.43 of what the rule
    allows), worst hop 1.7e-6 / 1.7e-6 / 4.0e-6."""
    seed = 9
    v = pkg.create_griffin_lim(iters=ITERS, seed=seed)
    try:
        v.set_opts(output_normalise=0, batch_shape=4 if form == "shape4" else 0)
        refs = batch_ref(orc, orc64, seed)
        mels = [m for _F, m, _a, _b in refs]
        force = {"shape4": None, "force42": "42", "force8": "8"}[form]
        with forced_env("XDTTS_GL", None), forced_env("XDTTS_GL_BATCH_FORCE", force):
            fwd = v.infer_batch(mels)
            rev = v.infer_batch(mels[::-1])[::-1]
        assert len(fwd) == len(rev) == len(refs)
        for order, got in (("fwd", fwd), ("rev", rev)):
            for (F, _mel, f32, f64), a in zip(refs, got):
                check_audio("batch/%s/%s" % (form, order), F, a, f32, f64)
        if form == "force8":  # (the 8-frame split really ran: another order of roundings than the 4-frame one)
            with forced_env("XDTTS_GL", None), forced_env("XDTTS_GL_BATCH_FORCE", "41"):
                four = v.infer_batch(mels)
            assert not all(np.array_equal(a, b) for a, b in zip(fwd, four))
        assert_no_fallback(capfd)
    finally:
        v.close()


@pytest.mark.parametrize("F", gs.SWEEP_SEEDED)
def test_seeded_phase_drawn_in_the_kernel(voc, orc, orc64, capfd, F):
    """(e) phase0 = None: k_gl_persistent draws the initial phase itself, keyed f * 513 + k with f the frame inside
    the utterance -- at a 3-frame-workgroup size and on the 5-wave launch.  MI355X: whole-signal rms 1.9e-7 / 2.4e-7,
    worst hop 3.3e-7 / 2.0e-6."""
    S = audio_ref(orc, orc64, F)[0]
    f32 = orc.griffinlim(S, seed=SEED, iters=ITERS)
    f64 = orc64.griffinlim(S, seed=SEED, iters=ITERS)
    voc.set_seed(SEED)
    with forced_env("XDTTS_GL", None):
        a = voc.infer_linear(S, iters=ITERS)
    check_audio("seeded", F, a, f32, f64)
    assert_no_fallback(capfd)
