"""GPU tests of the SPSI initial phase (phase_init mode 1, phase_spsi.hip): the hook against tests/spsi_ref.py bit for bit, the
ragged form against the single one, the mode's plumbing, its composition with the loop on both engines, the property the
stage exists for measured on the device, and the batch / sequence contracts in mode 1.

SPSI_L restates the segment length of the scan (magnitude_plan.h): the frame counts below are one segment, a partial last segment,
several segments, and more segments than one carry step."""
import os
import subprocess
import sys

import numpy as np
import pytest

import prosody_ref as pr
import spsi_ref as sr
from conftest import synth_ids

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPSI_L = 24
HOOK_FRAMES = (1, 2, 3, 5, SPSI_L - 1, SPSI_L, SPSI_L + 1, 2 * SPSI_L + 1, 4 * SPSI_L + 3, 257)
RAGGED_FRAMES = (1, 2 * SPSI_L + 1, 3, SPSI_L, 40)


def test_the_segment_length_is_the_librarys():
    with open(os.path.join(ROOT, "xd-tts_amd", "csrc", "magnitude_plan.h")) as f:
        assert "constexpr int SPSI_L = %d;" % SPSI_L in f.read()


@pytest.fixture(scope="module")
def voc(pkg):
    """Mode 0 until a test says otherwise (and every test that switches it switches it back)."""
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)
    v.set_opts(batch_shape=4)
    yield v
    v.close()


@pytest.fixture(scope="module")
def voc1(pkg):
    """A handle in mode 1 with the single call's split into workgroups (batch_shape 4: batches are bit for bit)."""
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)
    v.set_opts(batch_shape=4)
    v.set_phase_init(1)
    yield v
    v.close()


def hook_inputs(F):
    S = pr.random_magnitude(F, seed=700 + F)
    one = S.copy()
    one[:, F // 2] = 0.0
    first = S.copy()
    first[:, 0] = 0.0
    return (("random", S), ("one frame zero", one), ("first frame zero", first))


@pytest.mark.parametrize("F", HOOK_FRAMES)
def test_hook_against_the_reference(voc, F):
    """turns == spsi_ref bit for bit is what the definition promises when the fp32 division of p is correctly rounded (hipcc's
    default; the build uses no fast-math).  Asserted: the wrapped difference at frame t is at most 64 (t + 1) units -- 2 ulp of
    p, scaled by 2^30, per frame along the owner chain; whether it was 0 is printed.  angles against the fp64 (cos, sin) of
    the device's own turns: 4e-7, sincospif at a few ulp around 1.  MI355X: every case bit for bit, angles within 5.1e-8."""
    for name, S in hook_inputs(F):
        turns, ang = voc.spsi_phase(S)
        assert turns.shape == (513, F) and turns.dtype == np.uint32 and ang.shape == (513, F, 2) and ang.dtype == np.float32
        want = sr.turns(S)
        diff = (turns.astype(np.int64) - want.astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)
        worst = np.abs(diff).max(axis=0)  # per frame
        print("spsi hook F=%3d %-16s: max wrapped |turns - ref| %d units%s" % (F, name, worst.max(), " (bit for bit)" if not worst.max() else ""))
        assert (worst <= 64 * (np.arange(F) + 1)).all(), (F, name, worst)
        e = float(np.abs(ang.astype(np.float64) - sr.angles(turns)).max())
        print("spsi hook F=%3d %-16s: max |angles - fp64(turns)| %.2e" % (F, name, e))
        assert e <= 4e-7, (F, name, e)
        if name == "first frame zero":
            assert not turns[:, 0].any()  # carried through from phi_{-1} = 0
        if name == "one frame zero" and F >= 2:
            t = F // 2
            assert np.array_equal(turns[:, t], turns[:, t - 1])


def test_hook_on_an_all_zero_utterance(voc):
    turns, ang = voc.spsi_phase(np.zeros((513, SPSI_L + 2), dtype=np.float32))
    assert not turns.any() and np.array_equal(ang[..., 0], np.ones((513, SPSI_L + 2), dtype=np.float32)) and not ang[..., 1].any()


def test_ragged_hook_equals_the_single_hook(voc):
    mags = [pr.random_magnitude(F, seed=800 + u) for u, F in enumerate(RAGGED_FRAMES)]
    single = [voc.spsi_phase(S) for S in mags]
    for order in (range(len(mags)), reversed(range(len(mags)))):
        order = list(order)
        turns, angles = voc.spsi_phase_batch([mags[u] for u in order])
        for k, u in enumerate(order):
            assert turns[k].shape == (513, RAGGED_FRAMES[u]) and angles[k].shape == (513, RAGGED_FRAMES[u], 2)
            assert np.array_equal(turns[k], single[u][0]), (order, u)
            assert np.array_equal(angles[k], single[u][1]), (order, u)


def test_mode_plumbing(pkg, voc):
    assert voc.get_phase_init() == 0
    fresh = pkg.create_griffin_lim(iters=30, seed=3)
    try:
        assert fresh.get_phase_init() == 0
        for bad in (2, -1):
            with pytest.raises(pkg.XdttsError) as e:
                fresh.set_phase_init(bad)
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and fresh.get_phase_init() == 0
        fresh.set_phase_init(1)
        for bad in (2, -1):
            with pytest.raises(pkg.XdttsError) as e:
                fresh.set_phase_init(bad)
            assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and fresh.get_phase_init() == 1
        S = pr.random_magnitude(20, seed=5)
        spsi = fresh.infer_linear(S, iters=3)
        fresh.set_phase_init(0)
        assert fresh.get_phase_init() == 0
        back = fresh.infer_linear(S, iters=3)
        never = voc.infer_linear(S, iters=3)
        assert np.array_equal(back, never) and not np.array_equal(spsi, never)
    finally:
        fresh.close()


COMPOSITION = (
    "for F in (5, 48):\n"
    "    S = pr.random_magnitude(F, seed=500 + F)\n"
    "    ang = voc.spsi_phase(S)[1]\n"
    "    for K in (1, 5):\n"
    "        a = voc.infer_linear(S, iters=K)\n"
    "        b = voc.infer_linear(S, phase0=ang, iters=K)\n"
    "        assert a.shape == (256 * (F - 1),) and np.abs(a).max() > 0 and np.array_equal(a, b), (F, K)\n"
    "        print('spsi composition F=%d K=%d: bit for bit' % (F, K))\n"
)


def test_composition_with_the_loop(voc1):
    """Mode 1 is the stage followed by the route of a caller's phase0, on the persistent engine (F = 48; F = 5 runs the
    launch-per-iteration kernels on every handle) ..."""
    exec(COMPOSITION, {"pr": pr, "np": np, "voc": voc1})


def test_composition_with_the_loop_on_the_launch_engine():
    """... and with XDTTS_GL=launch, in a process of its own."""
    script = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import importlib\n"
        "import torch\n"
        "import numpy as np\n"
        "import prosody_ref as pr\n"
        "pkg = importlib.import_module('xd-tts_amd')\n"
        "voc = pkg.create_griffin_lim(iters=30, seed=3)\n"
        "voc.set_phase_init(1)\n" % (ROOT, os.path.join(ROOT, "tests"))
    ) + COMPOSITION + "print('SPSI LAUNCH OK')\n"
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, XDTTS_GL="launch"), capture_output=True, text=True, timeout=300)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "SPSI LAUNCH OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_the_property_on_the_device(voc, voc1):
    """On the voiced magnitude (F = 48, the device's own analysis) mode 1 reaches at most 0.6 x the spectral convergence of
    the seeded random start after 2 iterations and at most 0.8 x after 5 (the fp64 reference: 0.43 .. 0.50 and 0.45 .. 0.53,
    tests/test_spsi_cpu.py).  MI355X: 0.153 against 0.349 (0.44) and 0.124 against 0.251 (0.49)."""
    S, _ = voc.analyze(pr.voiced_signal(256 * 47), want_mel=False)
    assert S.shape == (513, 48)
    for K, factor in ((2, 0.6), (5, 0.8)):
        sc0 = voc.spectral_convergence(voc.infer_linear(S, iters=K), S)[0]
        sc1 = voc1.spectral_convergence(voc1.infer_linear(S, iters=K), S)[0]
        print("spsi property K=%d: mode 0 %.4f  mode 1 %.4f  ratio %.3f" % (K, sc0, sc1, sc1 / sc0))
        assert sc1 <= factor * sc0, (K, sc1, sc0)


@pytest.fixture(scope="module")
def mels():
    rng = np.random.default_rng(12)
    out = [(rng.uniform(-7.0, -1.0, size=(80, F)) + 2.0 * np.sin(np.arange(F) / 5.0)[None, :]).astype(np.float32) for F in (3, 48, 17)]
    for a in out:
        a.setflags(write=False)
    return out


def test_batch_equals_single_in_mode_1(voc, voc1, mels):
    one = [voc1.infer(m) for m in mels]
    for order in ((0, 1, 2), (2, 1, 0)):
        got = voc1.infer_batch([mels[u] for u in order])
        for k, u in enumerate(order):
            assert got[k].shape == (256 * (mels[u].shape[1] - 1),) and np.array_equal(got[k], one[u]), (order, u)
    t = voc1.last_timings()
    assert t["mel_to_linear_ms"] > 0 and t["iterations_ms"] > 0
    assert not np.array_equal(one[1], voc.infer(mels[1]))  # (the mode is in force: not the seeded stream's audio)


def test_batch_with_a_prosody_equals_single_in_mode_1(pkg, voc1, mels):
    ps = [pkg.Prosody(), pkg.Prosody(rate=1.25, pitch=0.8)]
    ms = [mels[2], mels[1]]
    one = [voc1.infer_prosody(m, p) for m, p in zip(ms, ps)]
    got = voc1.infer_batch(ms, prosody=ps)
    assert got[1].shape == (256 * (pkg.prosody_frames(48, 1.25) - 1),)
    for u in range(2):
        assert np.array_equal(got[u], one[u]), u
    assert np.array_equal(one[0], voc1.infer(ms[0]))


def test_sequence_equals_synthesize_in_mode_1(pkg, voc1, model):
    ids = [synth_ids(24, seed=s) for s in (2, 3)]
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    one = [pkg.synthesize(model, voc1, x, opts=opts) for x in ids]
    mels_, audios = pkg.synthesize_sequence(model, voc1, ids, opts=opts)
    for u in range(2):
        assert audios[u].shape == (256 * 39,) and np.array_equal(mels_[u], one[u][0]) and np.array_equal(audios[u], one[u][1]), u


def test_synthesize_batch_equals_its_two_halves_in_mode_1(pkg, voc1, model):
    groups = [[synth_ids(10, seed=2), synth_ids(8, seed=3)], [synth_ids(12, seed=6)]]
    steps = [[12, 14], [20]]
    opts = pkg.default_opts(dropout_seed=5)
    chunk_mels = model.infer_batch([c for g in groups for c in g], opts=opts, fixed_steps=[s for g in steps for s in g])
    want_mels = [np.concatenate(chunk_mels[0:2], axis=1), chunk_mels[2]]
    want_audio = voc1.infer_batch(want_mels)
    mels_, audios = pkg.synthesize_batch(model, voc1, groups, opts=opts, fixed_steps=steps)
    for u, F in enumerate((26, 20)):
        assert mels_[u].shape == (80, F) and np.array_equal(mels_[u], want_mels[u]), u
        assert audios[u].shape == (256 * (F - 1),) and np.array_equal(audios[u], want_audio[u]), u
