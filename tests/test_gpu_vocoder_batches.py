"""The utterance axis of a vocoder batch on the device: how gl_batch_plan packs a ragged batch into persistent launches
(tests/vocoder_batches.py restates it; test_vocoder_batches_cpu.py shows that these batches reach every class of plan on 256
CUs), through the loop and through both stage chains.  Every utterance of a case has its own mel, so a row, a segment or a
record that belongs to a neighbour changes the result.

  (a) the plan that ran        xdtts_griffinlim_batch_plan == the restatement, and the classes reached on this device
  (b) the loop                 every utterance against the fp64 oracle of ITS mel under the three rules of
                               test_gpu_griffinlim_shapes.check_audio; the 4-frame forms == the single call bit for bit
  (c) the delivery chain       launch by launch over permuted rows == the chain of the stages' own hooks on the raw audio,
                               audio and every stats struct, in the caller's order
  (d) the magnitude chain      batch == single bit for bit with F' frames, last_f0 / last_denoise in the caller's order
  (e) call order               one handle through requests of changing size == its first run and a fresh handle's

Four iterations and a fixed seed, as in test_gpu_griffinlim_shapes.py.  The figures of (b) are in profiles/vocoder_batches.txt
("vocoder-batches ..." lines: pytest -rA shows them for passing tests too)."""
import math

import numpy as np
import pytest

import gl_shapes as gs
import test_gpu_griffinlim_shapes as tgs
import vocoder_batches as vb
from gl_shapes import rms
from test_gpu_griffinlim_shapes import assert_no_fallback, forced_env

pytestmark = pytest.mark.gpu
ITERS = 4
SEED = 9
RATES = (8000, 48000)
LEVEL, LIM_US = (-23.0, -1.0), 5000   # LUFS, dBTP: on these signals the ceiling never binds
LOUD = (-10.0, -3.0)                  # ... and here it does: the limiter engages
SILENCE = dict(threshold_db=-6.0, min_sound_ms=10.0, lead_ms=5.0, trail_ms=5.0, max_pause_ms=20.0, fade_ms=2.0)  # trims edges: most of the signal lies 6 dB under its peak
TIMBRE = dict(vtl=1.12, breath=0.25, seed=9)
DENOISE = dict(strength=2.0, quantile=0.3, floor_db=-15.0, tone=[(300.0, -6.0), (3400.0, 0.0)])  # no profile: the selection runs


def _new(pkg):
    v = pkg.create_griffin_lim(iters=ITERS, seed=SEED)
    v.set_opts(output_normalise=0)
    return v


@pytest.fixture(scope="module")
def plain(pkg):
    """stages off: the single calls of (b), and the hooks of (c)"""
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = _new(pkg)
    yield v
    v.close()


class form_of:
    """A form of vocoder_batches.FORMS on a handle: batch_shape and the developer switch, the persistent engine allowed."""

    def __init__(self, v, form, gl=None):
        self.v, self.shape, self.force = v, vb.FORMS[form][0], vb.FORMS[form][1]
        self.env = [forced_env("XDTTS_GL", gl), forced_env("XDTTS_GL_BATCH_FORCE", None if self.force is None else str(self.force))]

    def __enter__(self):
        self.v.set_opts(batch_shape=self.shape)
        for e in self.env:
            e.__enter__()

    def __exit__(self, *exc):
        for e in self.env[::-1]:
            e.__exit__(*exc)
        self.v.set_opts(batch_shape=0)


def _plan_that_runs(v, Fu, form):
    """(what the device reports, the restatement at the CU figures it reports); they must agree"""
    bp = v.batch_plan(Fu)
    shape, force = vb.FORMS[form]
    p = vb.plan(Fu, bp["n_cu"], bp["per_cu4"], shape, force or 0)
    assert (bp["TF"], bp["WG"], bp["n_launches"], bp["launch_of"]) == (p.TF, p.WG, len(p.riders), vb.launch_of(p, len(Fu))), (form, bp, p.riders)
    return bp, p


_MELS, _REF, _SINGLE = {}, {}, {}


def mels_of(name):
    if name not in _MELS:
        _MELS[name] = vb.mels(name)
        for m in _MELS[name]:
            m.setflags(write=False)
    return _MELS[name]


def oracle_ref(orc, orc64, F, u):
    """Both oracles' audio from the oracle's own mel -> linear of speech_mel(F, seed=u): once per mel, never modified."""
    if (F, u) not in _REF:
        pinv = orc.pinv(orc.mel_filter_bank())
        S = orc.mel_to_linear(pinv, gs.speech_mel(F, seed=u), power=1.7)
        f32 = orc.griffinlim(S, seed=SEED, iters=ITERS)
        f64 = orc64.griffinlim(S, seed=SEED, iters=ITERS)
        for x in (f32, f64):
            x.setflags(write=False)
        _REF[(F, u)] = (f32, f64)
    return _REF[(F, u)]


def single_of(plain, name, u):
    """v.infer(mel) with every stage off, once per mel (C30's are C's)"""
    F = vb.CASES[name][u]
    if (F, u) not in _SINGLE:
        with forced_env("XDTTS_GL", None):
            a = plain.infer(mels_of(name)[u]).copy()
        a.setflags(write=False)
        _SINGLE[(F, u)] = a
    return _SINGLE[(F, u)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fields(s):
    vals = [getattr(s, name) for name, _ in s._fields_]
    return tuple(x.hex() if isinstance(x, float) else x for x in vals)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------

def test_the_plan_that_ran(pkg, plain, capfd):
    """(a) For every case and form the hook reports the plan of the restatement at the CU figures it reports; the classes of
    plan this device reaches are printed, and on 256 CUs with two 4-frame workgroups per CU they are all of them.  Under
    XDTTS_GL=launch the plan is empty.  The hook changes nothing and takes NULL for every output."""
    import ctypes as C

    reached, n_cu, per_cu4 = set(), None, None
    before = bytes(plain.get_opts())
    for name, Fu in vb.CASES.items():
        for form in vb.FORMS:
            with form_of(plain, form):
                bp, p = _plan_that_runs(plain, Fu, form)
            n_cu, per_cu4 = bp["n_cu"], bp["per_cu4"]
            reached |= vb.classes(p, Fu, n_cu)
        with form_of(plain, "41", gl="launch"):
            bp, p = _plan_that_runs(plain, Fu, "41")
        assert bp["n_cu"] == 0 and bp["n_launches"] == 0 and set(bp["launch_of"]) == {-1} and p.order == list(range(len(Fu)))
    assert bytes(plain.get_opts()) == before
    print("vocoder-batches classes reached on %d CUs, %d 4-frame workgroups per CU: %s" % (n_cu, per_cu4, " ".join(sorted(reached))))
    print("vocoder-batches classes not reached: %s" % (" ".join(sorted(vb.ALL_CLASSES - reached)) or "none"), flush=True)
    assert n_cu > 0, "no usable persistent engine on this device"
    if n_cu == 256 and per_cu4 >= 2:
        assert reached == vb.ALL_CLASSES, sorted(vb.ALL_CLASSES - reached)
    promised = set()
    for name, Fu in vb.CASES.items():
        for form in vb.FORMS:
            promised |= vb.classes(vb.case_plan(name, form, n_cu, per_cu4), Fu, n_cu)
    assert reached == promised
    nf = (C.c_size_t * 3)(40, 17, 5)
    assert pkg.lib.xdtts_griffinlim_batch_plan(plain._h, nf, 3, *([None] * 6)) == 0
    assert pkg.lib.xdtts_griffinlim_batch_plan(None, nf, 3, *([None] * 6)) == pkg.XDTTS_ERR_BAD_ARG
    assert pkg.lib.xdtts_griffinlim_batch_plan(plain._h, nf, 0, *([None] * 6)) == pkg.XDTTS_ERR_BAD_ARG
    assert_no_fallback(capfd)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------

LOOP_CASES = [(n, f) for n in ("A", "B", "D") for f in ("41", "8", "natural")] + [("C", "41"), ("C", "8")]


@pytest.mark.parametrize("name,form", LOOP_CASES)
def test_the_loop_against_fp64(pkg, plain, orc, orc64, capfd, name, form):
    """(b) Stages off.  One infer_batch forward and one reversed; each utterance against both oracles on ITS mel (check_audio's
    three rules, unchanged); where the plan's workgroups own 4 frames every audio is the single call's bit for bit, and the
    form 42 returns the bits of 41.  MI355X, worst of a case's utterances in both orders, against fp64 (the fp32 oracle's own
    figure in brackets; profiles/vocoder_batches.txt):
        case form     plan that ran             whole-signal rms       worst hop
        A    41       4x1, 3 launches, 1 alone  2.3e-7 (1.3e-7)        4.9e-6 (2.7e-6)
        A    8        8,   2 launches, 1 alone  2.5e-7 (1.3e-7)        5.3e-6 (2.7e-6)
        A    natural  4x2, 2 launches, 1 alone  2.3e-7 (1.3e-7)        4.9e-6 (2.7e-6)
        B    41       4x1, 3 launches, 2 alone  9.1e-7 (2.3e-7)        3.4e-6 (8.6e-7)   (F = 16 for both; 1100 alone: 5.4e-8)
        B    8        8,   2 launches, 1 alone  1.1e-7 (2.3e-7)        1.3e-6 (8.6e-7)
        B    natural  8,   2 launches, 1 alone  1.1e-7 (2.3e-7)        1.3e-6 (8.6e-7)
        C    41       4x1, 2 launches           5.3e-7 (7.3e-7)        2.7e-6 (3.6e-6)
        C    8        8,   2 launches           5.4e-7 (7.3e-7)        2.7e-6 (3.6e-6)
        D    41       4x1, 2 launches, 3 alone  1.1e-7 (1.7e-7)        1.5e-6 (2.4e-6)
        D    8        8,   2 launches, 2 alone  7.4e-8 (1.7e-7)        1.4e-6 (2.4e-6)
        D    natural  4x2, 1 launch,   3 alone  1.1e-7 (1.7e-7)        1.5e-6 (2.4e-6)
    No case failed when this test was written."""
    Fu, ms = vb.CASES[name], mels_of(name)
    n = len(Fu)
    refs = [oracle_ref(orc, orc64, F, u) for u, F in enumerate(Fu)]
    v = _new(pkg)
    try:
        worst = [0.0, 0.0, 0.0, 0.0]
        for order in ("fwd", "rev"):
            idx = list(range(n)) if order == "fwd" else list(range(n))[::-1]
            with form_of(v, form):
                bp, p = _plan_that_runs(v, [Fu[u] for u in idx], form)
                got = v.infer_batch([ms[u] for u in idx])
            assert len(got) == n
            if order == "fwd" and (name, form) in vb.QUOTED and bp["n_cu"] == 256 and bp["per_cu4"] >= 2:
                assert [len(r) for r in p.riders] == vb.QUOTED[(name, form)]
            for k, u in enumerate(idx):
                f32, f64 = refs[u]
                tgs.check_audio("batch/%s/%s/%s" % (name, form, order), Fu[u], got[k], f32, f64)
                worst = [max(worst[0], rms(got[k], f64)), max(worst[1], rms(f32, f64)), max(worst[2], gs.worst_hop(got[k], f64)), max(worst[3], gs.worst_hop(f32, f64))]
                if p.TF == 4 or not p.riders:
                    assert _same(got[k], single_of(plain, name, u)), (name, form, order, u, Fu[u])
            if form == "41" and order == "fwd":
                with form_of(v, "42"):
                    _plan_that_runs(v, Fu, "42")
                    two = v.infer_batch(ms)
                for u in range(n):
                    assert _same(two[u], got[u]), (name, u, Fu[u])
        print("vocoder-batches loop %-3s %-8s TF %d WG %d launches %d alone %d  rms gpu-f64 %.2e (f32-f64 %.2e)  worst hop gpu-f64 %.2e (f32-f64 %.2e)" % (
            name, form, p.TF, p.WG, len(p.riders), len(p.alone), worst[0], worst[1], worst[2], worst[3]), flush=True)
        assert_no_fallback(capfd)
    finally:
        v.close()


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------

def _delivery_on(pkg, v, rate, level=LEVEL):
    v.set_output_rate(rate)
    v.set_compressor(pkg.compressor_preset(1))
    v.set_loudness(*level)
    v.set_limiter(LIM_US)
    v.set_silence(pkg.Silence(**SILENCE))


def _delivery_off(v):
    v.set_output_rate(22050)
    v.set_compressor(None)
    v.set_loudness(None, None)
    v.set_limiter(0)
    v.set_silence(None)


def _delivery_stats(v):
    return [[_fields(s) for s in got] for got in (v.last_loudness(), v.last_limiter(), v.last_compressor(), v.last_silence())]


def chain_of_hooks(pkg, hook, raw, rate, level=LEVEL):
    """The delivery chain composed from the stages' own hooks, in delivery order: resample -> compress -> loudness (the gain
    rule of include/xdtts.h without the ceiling, which the limiter keeps) -> limit where it engages, else one fp32 factor ->
    trim.  Returns (audios, [loudness, limiter, compressor, silence] stats as _delivery_stats gives them, but for the gain)."""
    comp, sil = pkg.compressor_preset(1), pkg.Silence(**SILENCE)
    c_lin = math.pow(10.0, float(np.float32(level[1])) / 20.0)
    tgt = math.pow(10.0, (float(np.float32(level[0])) + 0.691) / 20.0)
    H = pkg.limiter_plan(rate, LIM_US)["half_width"]
    xs = hook.resample_batch(raw, rate)
    xs, cst = hook.compress_batch(xs, rate, comp)
    louds = hook.loudness_batch(xs, rate)
    ys, lst, gains = [], [], []
    for x, l in zip(xs, louds):
        Z, tp = l.mean_square, l.true_peak
        g0 = tgt / math.sqrt(Z) if Z > 0.0 else 1.0
        gains.append(g0)
        if Z > 0.0 and g0 * tp > c_lin:
            y, st = hook.limit(x, rate, g0, c_lin, LIM_US)
            assert st.engaged == 1
            lst.append(_fields(st))
        else:
            y = (x.astype(np.float32) * np.float32(g0)).astype(np.float32)
            lst.append(_fields(pkg.LimiterStats(1.0, H, 0, 0)))
        ys.append(y)
    outs, sst = hook.trim_batch(ys, rate, sil)
    return outs, [[_fields(l)[:3] + _fields(l)[4:] for l in louds], lst, [_fields(s) for s in cst], [_fields(s) for s in sst]], gains


def _delivery_case(pkg, hook, capfd, name, rate, form, gl=None, level=LEVEL):
    Fu, ms = vb.CASES[name], mels_of(name)
    n = len(Fu)
    v = _new(pkg)
    try:
        with form_of(v, form, gl=gl):
            bp, p = _plan_that_runs(v, Fu, form)
            raw = [a.copy() for a in v.infer_batch(ms)]
            assert _delivery_stats(v) == [[], [], [], []]
            _delivery_on(pkg, v, rate, level)
            assert _plan_that_runs(v, Fu, form)[0] == bp   # the plan does not depend on the stages
            got = [a.copy() for a in v.infer_batch(ms)]
            stats = _delivery_stats(v)
            if gl == "launch":
                assert bp["n_cu"] == 0 and not p.riders
            elif bp["n_cu"] == 256 and bp["per_cu4"] >= 2:
                assert [len(r) for r in p.riders] == vb.QUOTED[(name, form)] and p.order != list(range(n))
            want, wstats, gains = chain_of_hooks(pkg, hook, raw, rate, level)
            assert [len(s) for s in stats] == [n, n, n, n]
            for u in range(n):
                assert _same(got[u], want[u]), (name, rate, form, u, Fu[u], got[u].shape, want[u].shape)
                l = stats[0][u]
                assert l[:3] + l[4:] == wstats[0][u], (name, rate, form, u)
                g = float.fromhex(l[3])
                # the gain: 10^((T + 0.691) / 20) / sqrt(Z) in double -- pow of two C libraries may differ in the last place
                assert abs(g - gains[u]) <= 4.0 * 2.0 ** -52 * gains[u], (name, rate, form, u, g, gains[u])
                assert [stats[k][u] for k in (1, 2, 3)] == [wstats[k][u] for k in (1, 2, 3)], (name, rate, form, u)
            sil = v.last_silence()
            assert any(s.n_out < s.n_in for s in sil) and all(s.lead_cut + s.trail_cut + s.pause_cut + s.n_out == s.n_in for s in sil)
            assert len({a.shape for a in got}) > 1
            engaged = sum(s.engaged for s in v.last_limiter())   # (of the batch: the single calls below replace the tables)
            print("vocoder-batches delivery %-3s %5d Hz %-3s%s launches %d alone %d: of %d utterances %d levelled, %d under the limiter, %d trimmed" % (
                name, rate, form, " launch engine" if gl else "", len(p.riders), len(p.alone), n, sum(s.mean_square > 0 for s in v.last_loudness()),
                engaged, sum(s.n_out < s.n_in for s in sil)), flush=True)
            if p.TF == 4 or not p.riders:   # the single call's bits, audio and stats
                for u in range(n):
                    a = v.infer(ms[u])
                    assert _same(a, got[u]), (name, rate, form, u, Fu[u])
                    assert [s[0] for s in _delivery_stats(v)] == [stats[k][u] for k in range(4)], (name, rate, form, u)
        assert_no_fallback(capfd)
        return engaged
    finally:
        v.close()


@pytest.mark.parametrize("form", ["41", "42", "8"])
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", ["A", "C"])
def test_the_delivery_chain_over_permuted_rows(pkg, plain, capfd, name, rate, form):
    """(c) Output rate, compressor preset 1, -23 LUFS under -1 dBTP, limiter 5000 us and a silence setting that trims: the
    stages run once per launch over that launch's rows, which follow GlBatchPlan::order.  Delivered audio and all four stats
    tables == the chain of hooks on the same handle's raw audio, in the caller's order; under the 4-frame forms also the
    single call's."""
    _delivery_case(pkg, plain, capfd, name, rate, form)


@pytest.mark.parametrize("rate", RATES)
def test_the_delivery_chain_with_every_utterance_alone(pkg, plain, capfd, rate):
    """(c) case A, form 41 under XDTTS_GL=launch: the empty plan, five fetches of one row each."""
    _delivery_case(pkg, plain, capfd, "A", rate, "41", gl="launch")


@pytest.mark.parametrize("name", ["A", "C"])
def test_the_delivery_chain_under_an_engaged_limiter(pkg, plain, capfd, name):
    """(c) once more at -10 LUFS under -3 dBTP, form 41 at 8000 Hz: with the settings above the ceiling binds on no utterance
    (every row takes the one-factor branch), here the limiter's own rows and stats are under the permuted order too."""
    assert _delivery_case(pkg, plain, capfd, name, 8000, "41", level=LOUD) > 0


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------

def _contour(pkg, r):
    """a pitch ramp, a gain dip and a rate that is never 1"""
    return pkg.ProsodyContour([(0.0, r, 0.9, 1.0), (0.5, r * 1.04, 1.1, 0.7), (1.0, r, 1.25, 1.2)])


def _targets(pkg, n):
    kinds = [dict(hz=180.0), dict(factor=1.1, range=0.5), dict(hz=110.0, range=1.5), dict(factor=0.9)]
    return [pkg.PitchTarget(**kinds[u % 4]) for u in range(n)]


@pytest.mark.parametrize("name", ["A", "C30"])
def test_the_magnitude_chain(pkg, capfd, name):
    """(d) A pitch target over a contour whose rate is never 1, a timbre, a denoise with selection, SPSI initial phase: the loop
    runs on F' frames, and the packing works from F'.  Case A with rates 1.2 .. 1.32 (F' about 800: three launches under the
    form 41, asserted through the plan of the F' values) and the first 30 utterances of C with rates 0.8 .. 1.3: batch ==
    single bit for bit under 41 and 42, forward and reversed, last_f0 and last_denoise in the caller's order."""
    Fu, ms = vb.CASES[name], mels_of(name)
    n = len(Fu)
    rates = [1.2 + 0.03 * u for u in range(n)] if name == "A" else [(0.8, 1.3, 1.25, 0.9, 1.1)[u % 5] for u in range(n)]
    cons, tgts = [_contour(pkg, r) for r in rates], _targets(pkg, n)
    Fp = [pkg.prosody_contour_frames(c, F) for c, F in zip(cons, Fu)]
    assert all(a != b for a, b in zip(Fp, Fu))
    v = _new(pkg)
    try:
        v.set_timbre(pkg.Timbre(**TIMBRE))
        v.set_denoise(pkg.Denoise(**DENOISE))
        v.set_phase_init(1)
        single, f0, dn = [], [], []
        with forced_env("XDTTS_GL", None):
            for m, c, t, F, fp in zip(ms, cons, tgts, Fu, Fp):
                a = v.infer_pitch_target(m, t, c).copy()
                assert a.shape == (256 * (fp - 1),) and np.all(np.isfinite(a)) and np.any(a != 0)
                single.append(a)
                (s,), (d,) = v.last_f0(), v.last_denoise()
                assert s.n_frames == F and d.cells == 513 * F and d.rank == pkg.denoise_rank(F, DENOISE["quantile"]) and d.profiled == 0
                f0.append(_fields(s))
                dn.append(_fields(d))
        assert len(set(f0)) > 1 and len(set(dn)) > 1
        for form in ("41", "42"):
            for idx in (list(range(n)), list(range(n))[::-1]):
                with form_of(v, form):
                    bp, p = _plan_that_runs(v, [Fp[u] for u in idx], form)
                    if name == "A" and form == "41":
                        assert len(p.riders) >= 2, (Fp, p.riders)
                    assert p.riders and p.TF == 4
                    got = v.infer_batch_pitch_target([ms[u] for u in idx], [tgts[u] for u in idx], [cons[u] for u in idx])
                for k, u in enumerate(idx):
                    assert _same(got[k], single[u]), (name, form, idx[0], u, Fu[u], Fp[u])
                assert [_fields(s) for s in v.last_f0()] == [f0[u] for u in idx], (name, form, idx[0])
                assert [_fields(s) for s in v.last_denoise()] == [dn[u] for u in idx], (name, form, idx[0])
        assert_no_fallback(capfd)
    finally:
        v.close()


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------

SEQUENCE = (("C", "41", None), ("A", "8", None), ("single", None, None), ("B", "natural", None), ("A", "42", None), ("C", "41", None),
            ("D", "41", None), ("A", "41", "launch"))
SINGLE_F = 1026


def _run_step(pkg, v, step):
    name, form, gl = step
    if name == "single":
        with forced_env("XDTTS_GL", None):
            out = [v.infer(gs.speech_mel(SINGLE_F, seed=77)).copy()]
    else:
        with form_of(v, form, gl=gl):
            _plan_that_runs(v, vb.CASES[name], form)
            out = [a.copy() for a in v.infer_batch(mels_of(name))]
    return [_bits(a).tobytes() for a in out], _delivery_stats(v)


def test_call_order_on_one_handle(pkg, capfd):
    """(e) One handle, the delivery chain on at 8000 Hz, through C/41, A/8, a single infer of 1026 frames, B/natural, A/42, C/41,
    D/41, A/41 on the launch engine, then the same backwards: every result, audio and stats, equals its first run and a fresh
    handle's.  Between the calls the exchange buffer is reused under advancing epochs or grows, and the segment table, the
    copy events and the stages' record tables change size."""
    v = _new(pkg)
    try:
        _delivery_on(pkg, v, 8000)
        first = {}
        for step in SEQUENCE + SEQUENCE[::-1]:
            got = _run_step(pkg, v, step)
            if step not in first:
                first[step] = got
                fresh = _new(pkg)
                try:
                    _delivery_on(pkg, fresh, 8000)
                    assert _run_step(pkg, fresh, step) == got, step
                finally:
                    fresh.close()
            assert got == first[step], step
        assert_no_fallback(capfd)
    finally:
        v.close()
