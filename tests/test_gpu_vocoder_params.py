"""GPU parity of the vocoder across the constructor parameters xdtts_griffinlim_new accepts (tests/vocoder_params.py holds
the grid and the references; test_vocoder_params_cpu.py shows what the grid reaches): mel bases of 16 .. 128 bands -- every
K-slab class of k_gemm_nt from half a slab to four, the prologue's guarded 1- and 2-slab cases among them --, powers 1.0 / 1.7 /
2.0 / 0.6, momenta 0 / 0.5 / 0.99 and constructor iteration counts 0 / 1 / 2, each against the fp64 oracle; and what the
constructor and the xdtts_synthesize* entries refuse.

The rules are the suite's own, none is this file's:
  mel -> linear       worst frame against fp64 <= gemm_shapes.bound(d32) = 4 d32 + 1e-6
  analysis log-mel    max abs against the fp64 chain <= 4 d32 + 1e-6 (test_gpu_gemm_shapes.py); the magnitude under
                      test_gpu_analysis.py's rule (rms <= 2 x the fp32 oracle's + 1e-6 s, and <= 2e-5 s)
  audio               test_gpu_griffinlim_shapes.check_audio: rms against fp64 <= 2 x the fp32 oracle's + 1e-6, rms against the
                      fp32 oracle <= 1e-4, worst hop <= 1e-3 (every reference stays below 6e-5 there: the CPU file)
  step hook           test_gpu_griffinlim_shapes.test_step_hook: rebuilt spectrum and angles <= 2 x the fp32 oracle's + 1e-6,
                      every frame of the rebuilt spectrum <= 1e-4
Every test prints its figures ("vocoder-params ..." lines: pytest -rA shows them for passing tests too;
profiles/vocoder_params.txt holds those of an MI355X).  There, against fp64 (the fp32 oracle's own figure in brackets):
mel -> linear 5.0e-8 .. 3.6e-7 per frame (d32 4.4e-8 .. 3.7e-7, bound 1.2e-6 .. 2.5e-6) over all bases, powers and NNLS / exponent
modes; the analysis log-mel 1.0e-6 .. 2.0e-6 (1.5e-6 .. 2.1e-6) at 16 bands to 5.9e-5 (4.2e-5) at 128; the loop's audio 1.6e-8 ..
1.9e-7 rms (1.5e-8 .. 3.9e-7) with a worst hop of at most 8.9e-7 (1.1e-6); the step hook's rebuilt spectrum 1.6e-7 per frame
(1.7e-7) and angles 2.9e-6 .. 1.0e-5 (2.7e-6 .. 1.1e-5; closest to the rule at momentum 0.5, F = 17: 1.03e-5 against 2 x 7.6e-6 +
1e-6); end to end 2.2e-8 .. 7.5e-8 rms (1.9e-8 .. 1.9e-7)."""
import ctypes as C

import numpy as np
import pytest

import gemm_shapes as gs
import gl_shapes as gl
import vocoder_params as vp
from conftest import synth_ids
from test_gpu_griffinlim_shapes import FRAME_BOUND, HOP_BOUND, assert_no_fallback, forced_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make(pkg, orc):
    """make(key, power, iters, momentum): a handle of the grid, built once per parameter set and closed with the module."""
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    made = {}

    def get(key="m80", power=1.7, iters=2, momentum=0.99):
        k = (key, power, iters, momentum)
        if k not in made:
            made[k] = pkg.GriffinLim(vp.basis_pinv(orc, key)[0], vp.NOVERLAP, power, iters, momentum, seed=vp.SEED)
        return made[k]

    yield get
    for v in made.values():
        v.close()


def check_mel2lin(v, orc, orc64, key, F, power=1.7, nnls_iters=0, power_mode=0, tag="mel2lin"):
    mel, s64, d32 = vp.mel2lin_ref(orc, orc64, key, F, power=power, nnls_iters=nnls_iters, power_mode=power_mode)
    S = v.mel_to_linear(mel)
    assert S.shape == (vp.N_BINS, F) and S.dtype == np.float32 and np.all(np.isfinite(S)), (tag, key, F)
    e = gs.worst(S, s64, 0)
    names = ("mel2lin", "nnls_res", "nnls_upd") if nnls_iters else ("mel2lin",)
    print("vocoder-params %-8s %-6s F=%3d power %.1f nnls=%d mode=%d err(gpu,f64) %.2e (frame %d)  d32 %.2e  bound %.2e  %s" % (
        tag, key, F, power, nnls_iters, power_mode, e, int(np.argmax(gs.per_row_rel(S, s64, 0))), d32, gs.bound(d32),
        " ".join(vp.shape_class(key, s, F) for s in names)), flush=True)
    assert e <= gs.bound(d32), (tag, key, F, power, nnls_iters, power_mode, e, d32)


def check_audio(tag, F, a, f32, f64):
    """The assertions of test_gpu_griffinlim_shapes.check_audio; prints the figures first."""
    assert a.shape == (vp.HOP * (F - 1),) and a.dtype == np.float32, (tag, F, a.shape)
    assert np.all(np.isfinite(a)), (tag, F)
    eg, ef, e32, hg, hf = vp.audio_figures(a, f32, f64)
    print("vocoder-params %-28s F=%2d rms gpu-f64 %.2e  f32-f64 %.2e  gpu-f32 %.2e  worst hop gpu-f64 %.2e (hop %d)  f32-f64 %.2e" % (
        tag, F, eg, ef, e32, hg, int(np.argmax(gl.hop_rms(a, f64))), hf), flush=True)
    assert eg <= 2.0 * ef + 1e-6, (tag, F, eg, ef)
    assert e32 <= 1e-4, (tag, F, e32)
    assert hg <= HOP_BOUND, (tag, F, hg, int(np.argmax(gl.hop_rms(a, f64))))


# ---- 1. mel -> linear per basis ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(vp.BASES))
def test_mel_to_linear_per_basis(make, orc, orc64, key):
    """pinv . exp(mel) at F = 1, 31, 33, 70 (one row, a row tile short of / past 32, three row tiles) with K = n_mels columns:
    half a slab (16 bands) to four."""
    for F in vp.MEL2LIN_F:
        check_mel2lin(make(key), orc, orc64, key, F)


@pytest.mark.parametrize("power", [p for p in vp.POWERS if p != 1.7])
@pytest.mark.parametrize("key", vp.MEL2LIN_POWER_BASES)
def test_mel_to_linear_per_power(make, orc, orc64, key, power):
    """The other exponents of the epilogue: none at power 1, x^(1/2), x^(1/0.6)."""
    for F in vp.MEL2LIN_POWER_F:
        check_mel2lin(make(key, power=power), orc, orc64, key, F, power=power, tag="power")


@pytest.mark.parametrize("key,F", vp.MEL2LIN_XCD)
def test_mel_to_linear_row_tile_per_xcd(make, orc, orc64, key, F):
    """F = 520 > 513 rows: the row-tile-per-XCD mapping, 17 row tiles padded to 24, at the smallest and the largest K."""
    check_mel2lin(make(key), orc, orc64, key, F, tag="xcd")


@pytest.mark.parametrize("nnls_iters,power_mode", vp.NNLS_MODES)
@pytest.mark.parametrize("key", vp.NNLS_BASES)
def test_nnls_and_power_mode_per_basis(pkg, orc, orc64, key, nnls_iters, power_mode):
    """The refinement's residual GEMM (N = n_mels columns, K = 528) and update GEMM (K = n_mels) at F on both sides of the
    residual's flip rows > n_mels, and the exponent conventions 1 (x^power) and 2 (none)."""
    v = pkg.GriffinLim(vp.basis_pinv(orc, key)[0], vp.NOVERLAP, 1.7, 2, 0.99, seed=vp.SEED)
    try:
        v.set_opts(nnls_iters=nnls_iters, power_mode=power_mode)
        for F in vp.nnls_frames(key):
            check_mel2lin(v, orc, orc64, key, F, nnls_iters=nnls_iters, power_mode=power_mode, tag="nnls")
    finally:
        v.close()


# ---- 2. analysis per basis ----------------------------------------------------------------------------------------------

def check_analysis(v, orc, orc64, key, F, power=1.7):
    y, want, d32, m64, m32 = vp.analysis_ref(orc, orc64, key, F, power=power)
    S, mel = v.analyze(y)
    n = vp.n_mels_of(key)
    assert mel.shape == (n, F) and S.shape == (vp.N_BINS, F) and np.all(np.isfinite(mel)) and np.all(np.isfinite(S))
    dg = float(np.abs(mel - want).max())
    s = gl.rms(m64, 0 * m64)
    eg, ef = gl.rms(S, m64), gl.rms(m32, m64)
    print("vocoder-params analysis %-6s F=%3d power %.1f max|gpu-f64| %.2e  d32 %.2e  bound %.2e  magnitude err(gpu,f64)/s %.2e  err(orc32,f64)/s %.2e  %s" % (
        key, F, power, dg, d32, 4.0 * d32 + 1e-6, eg / s, ef / s, vp.shape_class(key, "analysis", F)), flush=True)
    assert dg <= 4.0 * d32 + 1e-6, (key, F, power, dg, d32)
    assert eg <= 2.0 * ef + 1e-6 * s and eg <= 2e-5 * s, (key, F, eg, ef, s)
    return S, mel


@pytest.mark.parametrize("key", vp.ANALYSIS_BASES)
def test_analysis_per_basis(make, orc, orc64, key):
    """analyze() at F = n_mels and n_mels + 1 frames: the projection (N = n_mels, K = 528) on the plain mapping and on the
    row-tile-per-XCD one; the log-mel has n_mels rows."""
    for F in vp.analysis_frames(key):
        check_analysis(make(key), orc, orc64, key, F)


@pytest.mark.parametrize("power", [1.0, 2.0])
def test_analysis_takes_the_handles_power(make, orc, orc64, power):
    check_analysis(make("m16", power=power), orc, orc64, "m16", 17, power=power)


@pytest.mark.parametrize("key", ["m16", "m128"])
def test_analysis_batch_row_order(make, orc, orc64, key):
    """Two utterances in one analyze_batch (their rows numbered through: n_mels + n_mels + 1 rows, past the flip): each is its
    single call bit for bit, in the caller's order, and both orders agree."""
    v = make(key)
    Fs = vp.analysis_frames(key)
    one = [check_analysis(v, orc, orc64, key, F) for F in Fs]
    ys = [vp.analysis_ref(orc, orc64, key, F)[0] for F in Fs]
    for order in ((0, 1), (1, 0)):
        S, mel = v.analyze_batch([ys[i] for i in order])
        for j, i in enumerate(order):
            assert np.array_equal(S[j], one[i][0]) and np.array_equal(mel[j], one[i][1]), (key, order, j)


# ---- 3. the loop per momentum and iteration count ----------------------------------------------------------------------------

@pytest.mark.parametrize("engine,F", [("default", F) for F in vp.LOOP_F] + [("launch", 40)])
@pytest.mark.parametrize("iters", vp.ITERS)
@pytest.mark.parametrize("momentum", vp.LOOP_MOMENTA)
def test_loop_per_momentum_and_iteration_count(make, orc, orc64, capfd, momentum, iters, engine, F):
    """infer_linear(iters=0) -- the handle's count, given to the constructor: 0 (the inverse STFT of S e^{i phase0}), 1 and 2 --
    from a fixed phase0, on the two-kernel path (F = 10), the persistent engine (17, 40) and XDTTS_GL=launch (40)."""
    S, p0, f32, f64 = vp.loop_ref(orc, orc64, F, momentum, iters)
    v = make(iters=iters, momentum=momentum)
    with forced_env("XDTTS_GL", "launch" if engine == "launch" else None):
        a = v.infer_linear(S, phase0=p0, iters=0)
    check_audio("loop/%s m=%.2f it=%d" % (engine, momentum, iters), F, a, f32, f64)
    assert_no_fallback(capfd)


@pytest.mark.parametrize("F", vp.LOOP_F)
@pytest.mark.parametrize("momentum", vp.MOMENTA)
def test_single_step_per_momentum(make, orc, orc64, capfd, momentum, F):
    """step(n_iter=1) from the fp32 oracle's state two iterations in (the momentum term live where there is one)."""
    S, a0, r0, (oa, orr), (da, dr) = vp.step_ref(orc, orc64, F, momentum)
    with forced_env("XDTTS_GL", None):
        ga, gr = make(momentum=momentum).step(S, a0, r0, n_iter=1)
    assert ga.shape == gr.shape == (vp.N_BINS, F, 2) and np.all(np.isfinite(ga)) and np.all(np.isfinite(gr))
    sig = float(np.sqrt(np.mean(dr ** 2)))
    eg, ef = gl.rms(gr, dr) / sig, gl.rms(orr, dr) / sig
    pg, pf = gl.per_frame_rel(gr, dr), gl.per_frame_rel(orr, dr)
    ag, af = gl.rms(ga, da), gl.rms(oa, da)
    print("vocoder-params step m=%.2f F=%2d rebuilt rel gpu-f64 %.2e  f32-f64 %.2e  per frame gpu-f64 %.2e (frame %d)  f32-f64 %.2e  "
          "angles gpu-f64 %.2e  f32-f64 %.2e" % (momentum, F, eg, ef, pg.max(), int(np.argmax(pg)), pf.max(), ag, af), flush=True)
    assert eg <= 2.0 * ef + 1e-6, (F, momentum, eg, ef)
    assert pg.max() <= FRAME_BOUND, (F, momentum, float(pg.max()), int(np.argmax(pg)))
    assert ag <= 2.0 * af + 1e-6, (F, momentum, ag, af)
    assert_no_fallback(capfd)


# ---- 4. end to end per basis ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(vp.BASES))
def test_end_to_end_per_basis(make, orc, orc64, capfd, key):
    """infer(mel) at F = 40, two iterations, the seeded phase drawn in the kernel, against the oracle from
    orc.phase_init(seed, 513, F)."""
    mel, f32, f64 = vp.e2e_ref(orc, orc64, key, vp.E2E_F)
    v = make(key)
    v.set_opts(output_normalise=0, batch_shape=0)
    v.set_seed(vp.SEED)
    with forced_env("XDTTS_GL", None):
        a = v.infer(mel)
    check_audio("e2e/%s" % key, vp.E2E_F, a, f32, f64)
    assert_no_fallback(capfd)


@pytest.mark.parametrize("key", vp.BATCH_BASES)
def test_batch_per_basis(make, orc, orc64, capfd, key):
    """infer_batch of F = 2, 17 and 40: the single calls bit for bit with batch_shape = 4, and inside the audio conditions with
    the default shape."""
    refs = [vp.e2e_ref(orc, orc64, key, F) for F in vp.BATCH_F]
    mels = [r[0] for r in refs]
    v = make(key)
    v.set_seed(vp.SEED)
    try:
        with forced_env("XDTTS_GL", None), forced_env("XDTTS_GL_BATCH_FORCE", None):
            v.set_opts(output_normalise=0, batch_shape=4)
            one = [v.infer(m) for m in mels]
            same = v.infer_batch(mels)
            v.set_opts(batch_shape=0)
            free = v.infer_batch(mels)
        assert len(same) == len(free) == len(mels)
        for F, a, b, c, (_m, f32, f64) in zip(vp.BATCH_F, one, same, free, refs):
            assert a.shape == b.shape and np.array_equal(a, b), (key, F)
            check_audio("batch/%s shape4" % key, F, b, f32, f64)
            check_audio("batch/%s default" % key, F, c, f32, f64)
    finally:
        v.set_opts(batch_shape=0)
    assert_no_fallback(capfd)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------

def refused_new(pkg, basis, power=1.7, iters=2, momentum=0.99):
    """xdtts_griffinlim_new through the C boundary: the status, the message, and the handle pointer it left."""
    b = np.ascontiguousarray(basis, dtype=np.float32)
    h = C.c_void_p(0xDEAD0)
    st = pkg.lib.xdtts_griffinlim_new(b.ctypes.data_as(C.c_void_p), b.shape[0], b.shape[1], vp.NOVERLAP, power, iters, momentum, 0, C.byref(h))
    return st, pkg.lib.xdtts_last_error().decode("utf-8", "replace"), h.value


def test_constructor_refusals(pkg, orc):
    """24 bands (no multiple of 16), the rank-deficient 160-band basis (named as such), power 0 / -1 / NaN / inf, momentum
    -0.1 / NaN (`momentum < 0` is false for a NaN, and every sample of every later call would be one): XDTTS_ERR_BAD_ARG and a
    null handle.  Before the checks were written, power = inf and momentum = NaN built a handle."""
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    B80 = vp.basis_pinv(orc, "m80")[0]
    cases = [("24 bands", dict(basis=orc.mel_filter_bank(n_mels=24)), "multiple of 16"),
             ("rank deficient", dict(basis=vp.rank_deficient_basis(orc)), "rank deficient")]
    cases += [("power %r" % p, dict(basis=B80, power=p), "power") for p in (0.0, -1.0, float("nan"), float("inf"), float("-inf"))]
    cases += [("momentum %r" % m, dict(basis=B80, momentum=m), "momentum") for m in (-0.1, float("nan"), float("inf"))]
    for tag, kw, word in cases:
        st, msg, h = refused_new(pkg, **kw)
        print("vocoder-params refusal %-18s status %d  %s" % (tag, st, msg), flush=True)
        assert st == pkg.XDTTS_ERR_BAD_ARG and h is None and word in msg, (tag, st, msg, h)
    # and the Python class raises the same
    with pytest.raises(pkg.XdttsError) as e:
        pkg.GriffinLim(B80, vp.NOVERLAP, 1.7, 2, float("nan"))
    assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    # the edges that are accepted: momentum 0 and 0 iterations build
    v = pkg.GriffinLim(B80, vp.NOVERLAP, 1.0, 0, 0.0)
    v.close()


def test_band_count_refusals_leave_the_handles_intact(pkg, model, orc):
    """A mel of the wrong row count into a handle, and a 64-band vocoder handed to the xdtts_synthesize* entries (which pass it
    the model's 80-row mel where it lies on the device): XDTTS_ERR_BAD_ARG naming both numbers, nothing returned -- and the
    same handles then deliver the bits of a pair that was never refused anything."""
    v80 = pkg.GriffinLim(vp.basis_pinv(orc, "m80")[0], vp.NOVERLAP, 1.7, 2, 0.99, seed=vp.SEED)
    v64 = pkg.GriffinLim(vp.basis_pinv(orc, "m64")[0], vp.NOVERLAP, 1.7, 2, 0.99, seed=vp.SEED)
    f80 = pkg.GriffinLim(vp.basis_pinv(orc, "m80")[0], vp.NOVERLAP, 1.7, 2, 0.99, seed=vp.SEED)
    f64 = pkg.GriffinLim(vp.basis_pinv(orc, "m64")[0], vp.NOVERLAP, 1.7, 2, 0.99, seed=vp.SEED)
    try:
        ids = [synth_ids(12, seed=31), synth_ids(9, seed=32)]
        o = pkg.default_opts(fixed_steps=10, dropout_seed=5)
        mel80, mel64 = vp.speech_mel("m80", 17), vp.speech_mel("m64", 17)
        want_mel, want_audio = pkg.synthesize(model, f80, ids[0], opts=o)  # the fresh pair, before anything is refused
        want64 = f64.infer(mel64)

        def refused(tag, call, *words):
            with pytest.raises(pkg.XdttsError) as e:
                call()
            print("vocoder-params refusal %-20s %s" % (tag, e.value), flush=True)
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and all(w in str(e.value) for w in words), (tag, str(e.value))

        def intact(tag):
            m, a = pkg.synthesize(model, v80, ids[0], opts=o)
            assert np.array_equal(m, want_mel) and np.array_equal(a, want_audio), tag
            assert np.array_equal(v64.infer(mel64), want64), tag

        intact("before")
        refused("mel80 -> 64 bands", lambda: v64.infer(mel80), "80", "64")
        intact("mel80 -> 64 bands")
        refused("mel64 -> 80 bands", lambda: v80.infer(mel64), "64", "80")
        intact("mel64 -> 80 bands")
        refused("mel80 -> 64 / batch", lambda: v64.infer_batch([mel80, mel80]), "80", "64")
        intact("mel80 -> 64 / batch")
        refused("synthesize", lambda: pkg.synthesize(model, v64, ids[0], opts=o), "64", "80")
        intact("synthesize")
        refused("synthesize_batch", lambda: pkg.synthesize_batch(model, v64, [[ids[0]], [ids[1]]], opts=o), "64", "80")
        intact("synthesize_batch")
        refused("synthesize_sequence", lambda: pkg.synthesize_sequence(model, v64, ids, None, opts=o), "64", "80")
        intact("synthesize_sequence")
        refused("synthesize_document", lambda: pkg.synthesize_document(model, v64, ids, opts=o), "64", "80")
        intact("synthesize_document")
        refused("synthesize / prosody", lambda: pkg.synthesize(model, v64, ids[0], opts=o, prosody=pkg.Prosody(rate=1.1, pitch=1.0)), "64", "80")
        intact("synthesize / prosody")
    finally:
        for v in (v80, v64, f80, f64):
            v.close()
