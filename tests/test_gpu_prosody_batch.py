"""GPU tests of the per-utterance prosody in the batch and sequence entries: the ragged kernel k_prosody_batch against the single
entry (bit for bit) and the fp64 restatement (tests/prosody_ref.py), the batched vocoder and the three pipeline entries against
their single-utterance forms, the all-identity calls against the plain entries, and the rejection of a bad array on live handles.

The test batch: F = 24, 40, 37, 20, 2, 3 frames at (rate, pitch) = (2, 1), (1.25, 0.8), (0.5, 1.3), identity, (4, 0.5), (0.25, 2),
i.e. F' = 13, 32, 73, 20, 2, 9 with the utterances' first output rows at 0, 13, 45, 118, 138, 140 and the end at 149: but for
140, no boundary is a multiple of the four frames of a workgroup, so four of the five boundaries lie inside a workgroup (one
workgroup, rows 136 .. 139, holds waves of two utterances with two rows each) and the batch ends on a partial workgroup.
Each utterance is scaled by another power of ten (1e-2 .. 1e3): a row read across a boundary cannot hide inside a tolerance."""
import ctypes as C

import numpy as np
import pytest

import prosody_ref as pr
from conftest import synth_ids

pytestmark = pytest.mark.gpu

FS = (24, 40, 37, 20, 2, 3)
RP = ((2.0, 1.0), (1.25, 0.8), (0.5, 1.3), (1.0, 1.0), (4.0, 0.5), (0.25, 2.0))
FP = (13, 32, 73, 20, 2, 9)


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)
    v.set_opts(batch_shape=4)  # the single call's split into workgroups: the batch's audio is the single call's bit for bit
    yield v
    v.close()


@pytest.fixture(scope="module")
def ps(pkg):
    return [pkg.Prosody(rate=r, pitch=p) for r, p in RP]


@pytest.fixture(scope="module")
def mags():
    """The six magnitudes (513, F_u), utterance u scaled by 10^(u - 2); read-only."""
    out = [(pr.random_magnitude(F, seed=300 + F) * np.float32(10.0 ** (u - 2))).astype(np.float32) for u, F in enumerate(FS)]
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def singles(voc, mags, ps):
    """prosody_linear on each utterance alone, computed once; read-only."""
    out = [voc.prosody_linear(S, p) for S, p in zip(mags, ps)]
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def mels():
    """Log-mels (80, F) of the first four frame counts, values as in test_identity_returns_the_bits_of_the_plain_entries."""
    rng = np.random.default_rng(11)
    out = [(rng.uniform(-7.0, -1.0, size=(80, F)) + 2.0 * np.sin(np.arange(F) / 5.0)[None, :]).astype(np.float32) for F in FS[:4]]
    for a in out:
        a.setflags(write=False)
    return out


def test_the_frame_counts_are_the_ones_the_cases_were_chosen_for(pkg):
    assert tuple(pkg.prosody_frames(F, r) for F, (r, _p) in zip(FS, RP)) == FP
    ends = [int(x) for x in np.cumsum(FP)]
    assert ends == [13, 45, 118, 138, 140, 149] and [x for x in ends if x % 4 == 0] == [140]


def test_hook_equals_the_single_entry_and_follows_fp64(pkg, voc, mags, ps, singles):
    """Bit for bit against prosody_linear per utterance, in both orders and for a batch of one; and, independently, within
    4 x d32 + 2e-5 of the fp64 reference (metric and bound of tests/test_gpu_prosody.py; d32 per case from the fp32 restatement,
    both relative to max(ref, log_floor) -- the scale of utterance u moves the cells against the fixed floor, which the metric
    takes in through its denominator)."""
    fwd = voc.prosody_linear_batch(mags, ps)
    rev = voc.prosody_linear_batch(mags[::-1], ps[::-1])[::-1]
    for u, (F, (rate, pitch)) in enumerate(zip(FS, RP)):
        one = voc.prosody_linear_batch([mags[u]], [ps[u]])[0]
        for name, out in (("forward", fwd[u]), ("reversed", rev[u]), ("alone", one)):
            assert out.shape == singles[u].shape == (513, FP[u]) and out.dtype == np.float32, (u, name)
            assert np.array_equal(out, singles[u]), (u, name)
        ref = pr.prosody(mags[u], rate, pitch)
        d32 = pr.rel_err(pr.prosody(mags[u], rate, pitch, dtype=np.float32), ref)
        err = pr.rel_err(fwd[u], ref)
        print("batch utterance %d F=%d F'=%d rate=%g pitch=%g: err(gpu) %.3e  d32 %.3e" % (u, F, FP[u], rate, pitch, err, d32))
        assert np.all(np.isfinite(fwd[u])) and err <= 4.0 * d32 + 2e-5, (u, err, d32)


def test_zeros_and_the_identity_inside_a_mix(pkg, voc, mags, ps):
    """The identity utterance comes back as it went in; a rate-only utterance with whole zero bins and zero columns has its
    zeros exactly where the reference has them; every cell of a pitch-changed utterance is finite and positive."""
    S = [a.copy() for a in mags]
    S[0][:12, :] = 0.0   # rate 2, pitch 1
    S[0][:, 10:13] = 0.0
    S[2][:12, :] = 0.0   # pitch 1.3
    S[2][:, 20:23] = 0.0
    out = voc.prosody_linear_batch(S, ps)
    assert np.array_equal(out[3], S[3]) and (S[3] == 0).any()
    ref = pr.prosody(S[0], *RP[0])
    assert (ref == 0).sum() > 12 * ref.shape[1] and np.array_equal(out[0] == 0, ref == 0)
    for u in (1, 2, 4, 5):
        assert np.all(np.isfinite(out[u])) and np.all(out[u] > 0), u


def test_batched_vocoder_equals_the_single_entry(pkg, voc, mels, ps):
    """infer_batch(mels, prosody=ps)[u] == infer_prosody(mels[u], ps[u]), both orders, 256 (F' - 1) samples.  F' = 13 runs
    alone (fewer than 16 frames), the others share persistent launches.  The existing pair infer_batch / infer on the same
    mels is measured beside it: the new pair is held to that pair's largest distance (0 where that pair is bit for bit)."""
    p4 = ps[:4]
    voc.set_seed(3)
    plain_one = [voc.infer(m) for m in mels]
    voc.set_seed(3)
    plain_batch = voc.infer_batch(mels)
    d_pair = max(float(np.abs(a - b).max()) for a, b in zip(plain_batch, plain_one))
    voc.set_seed(3)
    one = [voc.infer_prosody(m, p) for m, p in zip(mels, p4)]
    voc.set_seed(3)
    fwd = voc.infer_batch(mels, prosody=p4)
    t = voc.last_timings()
    voc.set_seed(3)
    rev = voc.infer_batch(mels[::-1], prosody=p4[::-1])[::-1]
    print("the pair infer_batch / infer without a prosody: max distance %.3e%s" % (d_pair, "" if d_pair else " (bit for bit)"))
    for u in range(4):
        assert one[u].shape == fwd[u].shape == rev[u].shape == (256 * (FP[u] - 1),), u
        d = max(float(np.abs(fwd[u] - one[u]).max()), float(np.abs(rev[u] - one[u]).max()))
        print("utterance %d F=%d F'=%d: max |batch - single| %.3e" % (u, FS[u], FP[u], d))
        assert np.all(np.isfinite(fwd[u])) and np.abs(fwd[u]).max() > 0 and d <= d_pair, (u, d, d_pair)
    assert t["mel_to_linear_ms"] > 0 and t["iterations_ms"] > 0  # ms[0]: mel -> linear and the stage


def test_last_timings_after_a_batch_with_a_prosody(pkg, voc, mels, ps):
    voc.infer_batch(mels[:2], prosody=ps[:2])
    t = voc.last_timings()
    assert t["mel_to_linear_ms"] > 0 and t["iterations_ms"] > 0 and t["total_ms"] >= t["iterations_ms"]


def test_all_identity_calls_return_the_bits_of_the_plain_entries(pkg, voc, mels, model):
    ident = [pkg.Prosody() for _ in range(4)]
    voc.set_seed(3)
    plain = voc.infer_batch(mels)
    voc.set_seed(3)
    with_p = voc.infer_batch(mels, prosody=ident)
    assert all(np.array_equal(a, b) for a, b in zip(plain, with_p))
    ids = [synth_ids(24, seed=s) for s in (2, 3, 4)]
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    voc.set_seed(3)
    m0, a0 = pkg.synthesize_sequence(model, voc, ids, opts=opts)
    voc.set_seed(3)
    m1, a1 = pkg.synthesize_sequence(model, voc, ids, opts=opts, prosody=ident[:3])
    assert all(np.array_equal(a, b) for a, b in zip(m0, m1)) and all(np.array_equal(a, b) for a, b in zip(a0, a1))
    assert all(a.shape == (256 * 39,) for a in a1)


def test_sequence_equals_synthesize_per_utterance(pkg, voc, model):
    ids = [synth_ids(24, seed=s) for s in (2, 3, 4)]
    sp = [pkg.Prosody(), pkg.Prosody(rate=1.25), pkg.Prosody(rate=0.7, pitch=1.3)]
    opts = pkg.default_opts(fixed_steps=40, dropout_seed=5)
    voc.set_seed(3)
    one = [pkg.synthesize(model, voc, x, opts=opts, prosody=p) for x, p in zip(ids, sp)]
    voc.set_seed(3)
    mels, audios = pkg.synthesize_sequence(model, voc, ids, opts=opts, prosody=sp)
    sizes = (256 * 39, 256 * 31, 256 * (pkg.prosody_frames(40, 0.7) - 1))
    for u in range(3):
        assert mels[u].shape == (80, 40) and audios[u].shape == (sizes[u],), u
        assert np.array_equal(mels[u], one[u][0]) and np.array_equal(audios[u], one[u][1]), u
    # the stop rule decides the frame count: no buffer can be sized beforehand
    mels, audios = pkg.synthesize_sequence(model, voc, ids, opts=pkg.default_opts(fixed_steps=0, max_steps=60, dropout_seed=5), prosody=sp)
    for u in range(3):
        F = mels[u].shape[1]
        assert 2 <= F <= 60 and audios[u].shape == (256 * (pkg.prosody_frames(F, sp[u].rate) - 1),) and np.all(np.isfinite(audios[u])), (u, F)


def test_synthesize_batch_equals_its_two_halves(pkg, voc, model):
    """synthesize_batch(prosody=ps) == tacotron2.infer_batch, the chunk mels of an utterance side by side, then
    infer_batch(mels, prosody=ps) -- the header's claim for the plain pair; the mels returned are the unmodified ones."""
    groups = [[synth_ids(10, seed=2), synth_ids(8, seed=3)], [synth_ids(9, seed=4), synth_ids(11, seed=5)], [synth_ids(12, seed=6)]]
    steps = [[12, 14], [16, 18], [20]]
    sp = [pkg.Prosody(rate=1.25, pitch=0.8), pkg.Prosody(), pkg.Prosody(rate=0.5)]
    opts = pkg.default_opts(dropout_seed=5)
    chunk_mels = model.infer_batch([c for g in groups for c in g], opts=opts, fixed_steps=[s for g in steps for s in g])
    want_mels = [np.concatenate(chunk_mels[0:2], axis=1), np.concatenate(chunk_mels[2:4], axis=1), chunk_mels[4]]
    voc.set_seed(3)
    want_audio = voc.infer_batch(want_mels, prosody=sp)
    voc.set_seed(3)
    mels, audios = pkg.synthesize_batch(model, voc, groups, opts=opts, fixed_steps=steps, prosody=sp)
    for u, F in enumerate((26, 34, 20)):
        assert mels[u].shape == (80, F) and np.array_equal(mels[u], want_mels[u]), u
        assert audios[u].shape == (256 * (pkg.prosody_frames(F, sp[u].rate) - 1),) and np.array_equal(audios[u], want_audio[u]), u


def test_a_bad_array_is_rejected_on_live_handles_and_nothing_is_returned(pkg, voc, model, mels):
    n = 3
    sp = (pkg.Prosody * n)(pkg.Prosody(rate=1.25), pkg.Prosody(pitch=2.5), pkg.Prosody())
    ms = [np.ascontiguousarray(m) for m in mels[:n]]
    ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in ms])
    nf = (C.c_size_t * n)(*[m.shape[1] for m in ms])
    audios, ns = (C.POINTER(C.c_float) * n)(), (C.c_size_t * n)(7, 7, 7)
    st = pkg.lib.xdtts_griffinlim_infer_batch_prosody(voc._h, ptrs, 80, nf, n, sp, audios, ns)
    assert st == pkg.XDTTS_ERR_BAD_ARG and b"pitch" in pkg.lib.xdtts_last_error() and b"utterance 1" in pkg.lib.xdtts_last_error()
    assert all(not audios[u] for u in range(n)) and list(ns) == [0, 0, 0]
    ids = [synth_ids(24, seed=s) for s in (2, 3, 4)]
    opts = pkg.default_opts(fixed_steps=12, dropout_seed=5)
    for call in (lambda p: pkg.synthesize_sequence(model, voc, ids, opts=opts, prosody=p),
                 lambda p: pkg.synthesize_batch(model, voc, [[x] for x in ids], opts=opts, prosody=p),
                 lambda p: voc.infer_batch(ms, prosody=p),
                 lambda p: voc.prosody_linear_batch([np.ones((513, 3), dtype=np.float32)] * n, p)):
        with pytest.raises(pkg.XdttsError) as e:
            call(list(sp))
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    with pytest.raises(pkg.XdttsError) as e:  # one frame, and not the identity
        voc.prosody_linear_batch([np.ones((513, 1), dtype=np.float32)] * 2, [pkg.Prosody(), pkg.Prosody(rate=2.0)])
    assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    # the handles still serve plain calls
    voc.set_seed(3)
    a = voc.infer_batch(ms)
    assert [x.size for x in a] == [256 * (m.shape[1] - 1) for m in ms]
    _m, a = pkg.synthesize_sequence(model, voc, ids[:2], opts=opts)
    assert [x.size for x in a] == [256 * 11] * 2
