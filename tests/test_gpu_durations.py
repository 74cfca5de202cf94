"""GPU tests of the durations stage (include/xdtts.h: per-id durations and timing marks from the cumulative attention): the stage
alone against the host reference bit for bit, every decoder engine against the fp64 oracle's cumulative weights after the same
steps, the row sums with the gate off and with the rigged gate on, batch against single, the bases of a three-chunk utterance,
and that the setting changes no mel bit and leaves the sequence entry alone.

Per-id bound, in frames, |dur - fp64 cumulative weight| <= BOUND: measured on an MI355X over the seven engine cases below (the
test prints every case's max and mean), with a margin of 4 for seeds and no more than test_durations_cpu.BOUND_CAP, against
which the discrimination of the CPU test was checked:

    case            engine        max         mean
    one             pair          7.066e-08   4.139e-08
    pair-unequal    pair          1.228e-07   3.515e-08
    pairs-B4        pair          1.619e-07   2.651e-08
    p8-B5           persistent8   1.320e-07   2.285e-08
    p16-B12         persistent8   1.187e-07   2.559e-08
    batched-B17     batched       2.963e-07   2.830e-08   (fast_exp in its softmax)
    launch-B2       launch        1.228e-07   3.752e-08
    BOUND = 1.2e-6 = 4 x 2.963e-07 rounded up; BOUND_CAP is 1e-4 (profiles/durations.txt has the same table from the tool).
No engine kept accumulating after a stop: the rigged-gate row sums hold on every engine."""
import numpy as np
import pytest

import decoder_steps as ds
import durations_ref as dr
from durations_ref import BOUND, EXPECT_ENGINE, MAX_STEPS, assert_same

pytestmark = pytest.mark.gpu

# the two-pair-launch form (XDTTS_P8=0: chunks 2 and 3 on views at b0 = 2) with the gate on -- not among decoder_steps' cases
ds.BY_NAME.setdefault("pairs-on-B4", ds.Case("pairs-on-B4", "p8off", (9, 6, 5, 12), gate=True))


def _handle(pkg, blob, form):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    with ds.form_env(form):
        return pkg.Tacotron2.from_blob(blob)


def _opts(pkg, **kw):
    return pkg.default_opts(dropout_seed=dr.DROPOUT_SEED, max_steps=MAX_STEPS, max_chunk=dr.WINDOW, **kw)


def _chunks(B):
    return [dr.case_ids(n, b) for b, n in enumerate(dr.case_lens(B))]


# ---- the stage alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("B", [1, 2, 17, 33])
def test_stage_alone_equals_the_host_reference(pkg, model, B, batched):
    """_durations_gather on crafted arrays: mixed parities, a permutation, ragged id counts, T in {24, 100, 512}, every chunk an
    utterance and utterances of three chunks -- every output and the stats, bit for bit."""
    rng = np.random.default_rng(100 * B + batched)
    for T, per_utt in ((24, 1), (100, 3), (512, 3)):
        cum_a = (rng.random((B, T)) * rng.choice([0.01, 1.0, 30.0], size=(B, 1))).astype(np.float32)
        cum_b = (rng.random((B, T)) * 5).astype(np.float32)
        cum_a[0, 0] = np.float32(2.5 / 65536)  # a tie
        nframes = rng.integers(0, 40, size=B).astype(np.int32)
        nframes[: B // 2] |= 1
        n_valid = rng.integers(1, T + 1, size=B).astype(np.int32)
        n_valid[-1] = T
        case = dict(cum_a=cum_a, cum_b=cum_b, nframes=nframes, n_valid=n_valid, order=rng.permutation(B).astype(np.int32), batched=batched,
                    utt_of_chunk=[c // per_utt for c in range(B)], opts=pkg.DurationsOpts(on=1, min_frames=0.25, max_frames=20.0))
        assert_same(model.durations_gather(**case), pkg.durations_reference(**case))
        assert model.last_durations_count() == 0  # a hook is no request


def test_two_utterances_of_three_chunks(pkg, model):
    rng = np.random.default_rng(5)
    cum = (rng.random((6, 24)) * 4).astype(np.float32)
    case = dict(cum_a=cum, cum_b=cum[::-1].copy(), nframes=[5, 8, 7, 12, 6, 9], n_valid=[24, 3, 17, 1, 24, 10], order=[4, 2, 0, 5, 1, 3],
                batched=True, utt_of_chunk=[0, 0, 0, 1, 1, 1])
    got = model.durations_gather(**case)
    assert_same(got, pkg.durations_reference(**case))
    assert_same(got, dr.durations(**{k: v for k, v in case.items()}))
    assert len(got[3]) == 2 and got[3][0].n_frames + got[3][1].n_frames == 47


# ---- every engine, fixed steps -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c[0] for c in dr.ENGINE_CASES])
def test_every_engine_matches_the_fp64_cumulative_weights(pkg, orc64, blob, name):
    _n, form, steps = [c for c in dr.ENGINE_CASES if c[0] == name][0]
    B = len(steps)
    assert ds.engine_for(B, dr.WINDOW, max(steps), form) == EXPECT_ENGINE[name]
    lens, chunks = dr.case_lens(B), _chunks(B)
    m = _handle(pkg, blob, form)
    try:
        m.set_durations(on=1)
        with ds.form_env(form):
            mels = m.infer_batch(chunks, opts=_opts(pkg), fixed_steps=np.asarray(steps, dtype=np.int32))
        assert [x.shape[1] for x in mels] == list(steps)
        assert m.last_durations_count() == B
        errs = []
        for b in range(B):
            dur, q, st = m.last_durations(b)
            s = m.last_alignment(b)
            want = dr.oracle_cum(orc64, blob, lens[b], b, steps[b])[0][:lens[b]]
            assert dur.shape == (lens[b],) and np.all(np.isfinite(dur))
            errs.append(np.abs(dur.astype(np.float64) - want))
            # row sum: the softmax rows sum to one
            assert abs(float(dur.astype(np.float64).sum()) - steps[b]) <= 1e-3 * steps[b], (name, b, float(dur.sum()), steps[b])
            assert np.array_equal(q, dr.q16(dur)) and st[0] == 0 and np.array_equal(st[1:], np.cumsum(q.astype(np.uint64))[:-1])
            assert (s.n_ids, s.n_frames, s.sum_q16, s.last_q16) == (lens[b], steps[b], int(q.astype(np.uint64).sum()), int(q[-1]))
        e = np.concatenate(errs)
        print("durations %-14s %-11s B=%2d steps %s  per-id |dur - f64| max %.3e mean %.3e bound %.1e" % (
            name, EXPECT_ENGINE[name], B, list(steps), e.max(), e.mean(), BOUND), flush=True)
        assert e.max() <= BOUND, (name, float(e.max()))
    finally:
        m.close()


# ---- the gate on -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["one-on-21", "pair-on-2-22", "pairs-on-B4", "p8-on-B5", "p8-on-B9", "batched-on-B17-last-tile-outlives", "launch-on-48-one-at-cap"])
def test_rigged_gate_row_sums_hold_against_the_returned_frame_counts(pkg, orc, orc64, blob, name):
    """Chunks stopping at different frames (decoder_steps' rigged gate): an engine that kept accumulating after a stop fails."""
    case = ds.BY_NAME[name]
    weights = ds.rigged(orc, orc64, blob, case)[0]
    m = _handle(pkg, weights, case.form)
    try:
        m.set_durations(on=1)
        mels = ds.run_case(pkg, m, case)
        assert [x.shape[1] for x in mels] == list(case.ends)
        assert m.last_durations_count() == case.B
        for b in range(case.B):
            dur, _q, _st = m.last_durations(b)
            F = mels[b].shape[1]
            assert dur.shape == (case.lens[b],)
            assert abs(float(dur.astype(np.float64).sum()) - F) <= 1e-3 * F, (name, b, float(dur.sum()), F)
            assert m.last_alignment(b).n_frames == F
    finally:
        m.close()


# ---- batch against single, order, bases --------------------------------------------------------------------------------------

def test_batch_of_17_against_the_chunks_one_by_one(pkg, blob):
    _n, form, steps = [c for c in dr.ENGINE_CASES if c[0] == "batched-B17"][0]
    B, chunks = len(steps), _chunks(len(steps))
    m = _handle(pkg, blob, form)
    try:
        m.set_durations(on=1)
        m.infer_batch(chunks, opts=_opts(pkg), fixed_steps=np.asarray(steps, dtype=np.int32))
        batch = [m.last_durations(b) for b in range(B)]
        for b in range(B):
            m.infer_batch([chunks[b]], opts=_opts(pkg, item_base=b), fixed_steps=np.asarray([steps[b]], dtype=np.int32))
            assert m.last_durations_count() == 1
            dur, q, st = m.last_durations(0)
            bdur, bq, bst = batch[b]
            # the layout, exactly: the id counts, and every start the prefix sum of the utterance's own Q16 durations from 0
            assert dur.shape == bdur.shape == q.shape == bq.shape == st.shape == bst.shape == (len(chunks[b]),)
            assert m.last_alignment(0).n_ids == len(chunks[b]) and m.last_alignment(0).n_frames == steps[b]
            for one_q, one_st in ((q, st), (bq, bst)):
                assert np.array_equal(one_st - one_st[0], np.concatenate([[0], np.cumsum(one_q.astype(np.uint64))[:-1]]).astype(np.uint64)) and one_st[0] == 0
            assert np.abs(dur.astype(np.float64) - bdur).max() <= BOUND, (b, float(np.abs(dur.astype(np.float64) - bdur).max()))
    finally:
        m.close()


def test_three_chunks_of_one_utterance_have_the_frame_count_prefix_as_bases(pkg, blob):
    lens = list(dr.UTT3_LENS)
    ids = np.concatenate([dr.case_ids(n, b) for b, n in enumerate(lens)])
    splits = np.cumsum(lens)[:-1]
    m = _handle(pkg, blob, "default")
    try:
        m.set_durations(on=1)
        mel = m.infer(ids, splits=splits, opts=_opts(pkg, fixed_frames_per_id=0.5))  # 5, 7 and 6 frames
        assert mel.shape[1] == 18 and m.last_durations_count() == 1
        dur, q, st = m.last_durations(0)
        s = m.last_alignment(0)
        assert dur.shape == (36,) and (s.n_ids, s.n_frames) == (36, 18)
        assert [int(st[0]), int(st[10]), int(st[24])] == [0, 5 * 65536, 12 * 65536]
        for a, e in ((0, 10), (10, 24), (24, 36)):
            assert np.array_equal(st[a:e] - st[a], np.concatenate([[0], np.cumsum(q[a:e].astype(np.uint64))[:-1]]).astype(np.uint64))
        with pytest.raises(pkg.XdttsError):
            m.last_durations(1)
    finally:
        m.close()


# ---- off is off ----------------------------------------------------------------------------------------------------------------

def test_the_setting_changes_no_bit_and_the_sequence_entry_ignores_it(pkg, blob):
    steps = np.asarray([6, 11, 5, 9, 7, 8], dtype=np.int32)
    chunks = _chunks(6)
    ids = np.concatenate(chunks[:3])
    splits = np.cumsum([len(c) for c in chunks[:3]])[:-1]
    m = _handle(pkg, blob, "default")
    voc = pkg.create_griffin_lim(iters=4, seed=3)
    try:
        assert m.get_durations().on == 0
        o = _opts(pkg, fixed_frames_per_id=0.5)
        off = (m.infer_batch(chunks, opts=_opts(pkg), fixed_steps=steps), m.last_durations_count(), m.infer(ids, splits=splits, opts=o), m.last_durations_count())
        seq_off = pkg.synthesize_sequence(m, voc, [ids, chunks[3]], [splits, None], opts=o)
        assert off[1] == 0 and off[3] == 0 and m.last_durations_count() == 0
        m.set_durations(on=1)
        assert m.get_durations().on == 1
        on = (m.infer_batch(chunks, opts=_opts(pkg), fixed_steps=steps), m.last_durations_count(), m.infer(ids, splits=splits, opts=o), m.last_durations_count())
        assert on[1] == 6 and on[3] == 1
        assert all(np.array_equal(a, b) for a, b in zip(off[0], on[0])) and np.array_equal(off[2], on[2])
        seq_on = pkg.synthesize_sequence(m, voc, [ids, chunks[3]], [splits, None], opts=o)
        assert m.last_durations_count() == 0
        for a, b in zip(seq_off[0] + seq_off[1], seq_on[0] + seq_on[1]):
            assert np.array_equal(a, b)
        # the synthesize entries are covered: one utterance / as utt_chunks says
        mel, _audio = pkg.synthesize(m, voc, ids, splits=splits, opts=o)
        assert m.last_durations_count() == 1 and np.array_equal(mel, on[2]) and m.last_alignment(0).n_frames == mel.shape[1]
        pkg.synthesize_batch(m, voc, [chunks[:2], chunks[2:3], chunks[3:]], opts=_opts(pkg), fixed_steps=[[6, 11], [5], [9, 7, 8]])
        assert m.last_durations_count() == 3
        assert [m.last_alignment(u).n_frames for u in range(3)] == [17, 5, 24]
        assert [m.last_durations(u)[0].size for u in range(3)] == [sum(len(c) for c in g) for g in (chunks[:2], chunks[2:3], chunks[3:])]
        m.set_durations()  # the default: off again
        m.infer_batch(chunks[:1], opts=_opts(pkg), fixed_steps=steps[:1])
        assert m.last_durations_count() == 0
    finally:
        voc.close()
        m.close()


# ---- id-anchored contours ------------------------------------------------------------------------------------------------------

def _mapped(pkg, m, u, F, points):
    """the host's mapping of id-anchored points through last_durations of utterance u: xdtts_durations_position, the running
    maximum, fp32"""
    _dur, q, st = m.last_durations(u)
    pos = np.maximum.accumulate([pkg.durations_position(st, q, F, float(p[0])) for p in points])
    return [(float(np.float32(x)),) + tuple(p[1:]) for x, p in zip(pos, points)]


def test_id_anchored_contour_equals_the_contour_entry_with_host_mapped_fractions(pkg, blob):
    lens = list(dr.UTT3_LENS)
    ids = np.concatenate([dr.case_ids(n, b) for b, n in enumerate(lens)])
    splits = np.cumsum(lens)[:-1]
    points = [(0, 1, 1, 1), (10, 1, 1, 1), (10, 1.25, 1.2, 0.8), (24.5, 0.8, 0.9, 1.0), (30, 1, 1, 1), (36, 1, 1, 1)]
    m = _handle(pkg, blob, "default")
    voc = pkg.create_griffin_lim(iters=4, seed=3)
    try:
        o = _opts(pkg, fixed_frames_per_id=0.5)
        m.set_durations(on=1)
        mel0, audio0 = pkg.synthesize(m, voc, ids, splits=splits, opts=o)
        mapped = _mapped(pkg, m, 0, mel0.shape[1], points)
        assert 0.0 == mapped[0][0] < mapped[1][0] == mapped[2][0] < mapped[3][0] < mapped[4][0] < mapped[5][0] <= 1.0
        assert abs(mapped[1][0] - 5 / 17) < 1e-6  # id 10 opens chunk 1: its base is chunk 0's 5 frames, of F - 1 = 17
        mel1, audio1 = pkg.synthesize(m, voc, ids, splits=splits, opts=o, contour=pkg.ProsodyContour(mapped))
        m.set_durations()  # off: the id-anchored entry captures whatever the setting says
        mel2, audio2 = pkg.synthesize(m, voc, ids, splits=splits, opts=o, contour_at_ids=pkg.ProsodyContour(points))
        assert m.last_durations_count() == 1 and m.last_durations(0)[0].shape == (36,)
        assert np.array_equal(mel1, mel2) and np.array_equal(mel0, mel2)
        assert audio1.shape == audio2.shape and np.array_equal(audio1, audio2)
        assert audio1.shape != audio0.shape or not np.array_equal(audio1, audio0)  # the contour does something
        # an all-identity contour: the plain call's bits
        mel3, audio3 = pkg.synthesize(m, voc, ids, splits=splits, opts=o, contour_at_ids=pkg.ProsodyContour([(0, 1, 1, 1), (18.5, 1, 1, 1), (36, 1, 1, 1)]))
        assert np.array_equal(mel3, mel0) and np.array_equal(audio3, audio0)
        with pytest.raises(pkg.XdttsError) as e:
            pkg.synthesize(m, voc, ids, splits=splits, opts=o, contour_at_ids=pkg.ProsodyContour([(0, 1, 1, 1), (36.5, 1, 1.2, 1)]))
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and "point 1" in str(e.value)
    finally:
        voc.close()
        m.close()


def test_id_anchored_contours_of_a_batch_equal_the_batch_contour_entry(pkg, blob):
    chunks = _chunks(6)
    utts, steps = [chunks[:2], chunks[2:3], chunks[3:]], [[6, 11], [5], [9, 7, 8]]
    n = [sum(len(c) for c in u) for u in utts]
    points = [[(0, 1, 1, 1), (len(chunks[0]), 1.25, 1.1, 1), (n[0], 0.8, 1, 1)],
              [(0, 1, 1, 1), (n[1], 1, 1, 1)],  # the identity inside a mixed batch
              [(1.5, 1, 0.9, 1), (n[2] - len(chunks[5]), 1, 0.9, 0.5), (n[2] - 0.25, 1.5, 1.2, 1)]]
    m = _handle(pkg, blob, "default")
    voc = pkg.create_griffin_lim(iters=4, seed=3)
    try:
        m.set_durations(on=1)
        mels0, audios0 = pkg.synthesize_batch(m, voc, utts, opts=_opts(pkg), fixed_steps=steps)
        mapped = [pkg.ProsodyContour(_mapped(pkg, m, u, mels0[u].shape[1], points[u])) for u in range(3)]
        mels1, audios1 = pkg.synthesize_batch(m, voc, utts, opts=_opts(pkg), fixed_steps=steps, contour=mapped)
        m.set_durations()
        mels2, audios2 = pkg.synthesize_batch(m, voc, utts, opts=_opts(pkg), fixed_steps=steps, contour_at_ids=[pkg.ProsodyContour(p) for p in points])
        assert m.last_durations_count() == 3
        for u in range(3):
            assert np.array_equal(mels1[u], mels2[u]) and np.array_equal(mels0[u], mels2[u])
            assert audios1[u].shape == audios2[u].shape and np.array_equal(audios1[u], audios2[u])
        assert np.array_equal(audios2[1], audios0[1]) and audios2[0].shape != audios0[0].shape
    finally:
        voc.close()
        m.close()
