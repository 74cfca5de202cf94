"""The frame counts that test_gpu_griffinlim_shapes.py sweeps reach every engine and every work split the
vocoder can choose on a 256-CU device.  This checks the LIST (against tests/gl_shapes.py's restatement of
the rules, and that restatement against the constants in the sources), not the kernels."""
import os
import re

import numpy as np
import pytest

import gl_shapes as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
N_CU = 256  # MI355X


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restated_rules_use_the_constants_of_the_sources():
    assert int(re.search(r"constexpr int GLP_TF_MAX = (\d+);", _src("gl_plan.h")).group(1)) == gs.GLP_TF_MAX == 8
    assert int(re.search(r"constexpr int FRAMES_PER_BLOCK = (\d+);", _src("gl_fft.h")).group(1)) == 4
    hop = re.search(r"constexpr int NFFT = (\d+), HOP = (\d+);", _src("gl_fft.h"))
    assert (int(hop.group(1)), int(hop.group(2))) == (2 * (gs.N_BINS - 1), gs.HOP)
    gl, plan = _src("griffinlim.hip"), _src("gl_plan.h")
    body = plan[plan.index("bool gl_persistent_plan("):]
    body = body[:body.index("\n}")]
    assert "if (F < %d) return false;" % gs.TINY_BELOW in body
    assert "std::max(4, (F + n_cu - 1) / n_cu)" in body and "if (tf > GLP_TF_MAX) return false;" in body
    assert "(F + tf - 1) / tf" in body and "nb > n_cu || F / nb < %d" % gs.MIN_OWN in body
    assert "if (g.F >= %d)" % gs.TINY_BELOW in gl  # launch_gl_iterate: fused kernel from 16 frames on
    assert "return (int)(((long long)b * F) / nblk);" in gl  # glp_fstart
    assert "return (int)(((long long)b * F) / nblk);" in plan  # gl_fstart, the header's statement of the same rule
    assert "Fu[u] < %d || nb > n_cu || Fu[u] / nb < %d" % (gs.TINY_BELOW, gs.MIN_OWN) in plan  # gl_batch_pack


def test_plan_at_the_thresholds():
    assert gs.plan(15, N_CU)[0] == "tiny" and gs.plan(16, N_CU) == ("p4", 4, [4, 4, 4, 4])
    assert gs.plan(1024, N_CU) == ("p4", 4, [4] * 256)
    assert gs.plan(1025, N_CU)[:2] == ("p8", 5) and gs.plan(2048, N_CU) == ("p8", 8, [8] * 256)
    assert gs.plan(2049, N_CU)[0] == "launch" and gs.plan(2049, N_CU)[2][-1] == 1
    for F, tf in ((1026, 5), (1281, 6), (1537, 7), (1793, 8)):
        engine, got, own = gs.plan(F, N_CU)
        assert (engine, got) == ("p8", tf) and sorted(set(own)) == [tf - 1, tf], (F, got, sorted(set(own)))


def test_every_own_count_is_at_least_three_and_they_sum_to_F():
    for F in sorted(set(gs.SWEEP_DEFAULT + gs.SWEEP_LAUNCH + gs.SWEEP_STEP + gs.SWEEP_SEEDED)):
        engine, tf, own = gs.plan(F, N_CU)
        assert sum(own) == F, F
        if engine in ("p4", "p8"):
            assert gs.MIN_OWN <= min(own) and max(own) <= tf <= gs.GLP_TF_MAX and len(own) <= N_CU, (F, tf, own)
    # and for every frame count the persistent engine takes at all, on this and on smaller devices
    for n_cu in (256, 128, 64, 8):
        for F in range(16, gs.GLP_TF_MAX * n_cu + 2):
            engine, tf, own = gs.plan(F, n_cu)
            assert sum(own) == F
            if engine in ("p4", "p8"):
                assert min(own) >= gs.MIN_OWN and max(own) <= tf and len(own) <= n_cu, (n_cu, F)
            else:
                assert engine == "launch" and (F > gs.GLP_TF_MAX * n_cu or F // -(-F // max(4, -(-F // n_cu))) < gs.MIN_OWN), (n_cu, F)


REQUIRED = {"tiny", "p4-all4", "p4-3-first-only", "p4-3-inside", "p8-tf5-mixed", "p8-tf6-mixed", "p8-tf7-mixed", "p8-tf8-mixed", "p8-tf8-even", "launch"}


def test_the_default_sweep_reaches_every_class():
    got = {}
    for F in gs.SWEEP_DEFAULT:
        got.setdefault(gs.shape_class(F, N_CU), []).append(F)
    assert set(got) == REQUIRED, (sorted(REQUIRED - set(got)), sorted(set(got) - REQUIRED))
    assert 15 in got["tiny"] and 10 in got["tiny"] and got["launch"] == [2049]
    # every class any frame count can produce is one of these: the list leaves none out
    # (an evenly split launch of 5, 6 or 7 frames per workgroup, F = 1030 say, has only the full workgroups that the mixed
    # split of the same TF has too)
    every = {gs.shape_class(F, N_CU) for F in range(2, 2200)}
    assert every - REQUIRED == {"p8-tf5-even", "p8-tf6-even", "p8-tf7-even"} and REQUIRED <= every, sorted(every ^ REQUIRED)


def test_a_three_frame_workgroup_is_never_the_last_one():
    """The floor split hands workgroup 0 floor(F / nblk) frames and the last one ceil(F / nblk): "a 3 at the last
    workgroup" does not occur for any F, alone or in a batch, so the sweep has no such case; the 3-frame
    workgroups it reaches are the first one (F = 19, 203) and the first plus inner ones (F = 17, 18, 21, 37)."""
    for F in range(16, 1025):
        engine, tf, own = gs.plan(F, N_CU)
        if engine == "p4" and F % 4:
            assert own[0] == 3 and own[-1] == 4, (F, own)
        split = gs.batch_split(F, 4, N_CU)
        if split is not None and F % 4:
            assert split[0] == 3 and split[-1] == 4, (F, split)
    assert gs.plan(19, N_CU)[2] == [3, 4, 4, 4, 4] and gs.plan(17, N_CU)[2] == [3, 3, 4, 3, 4]
    assert gs.plan(203, N_CU)[2] == [3] + [4] * 50
    assert gs.plan(37, N_CU)[2].count(3) == 3 and gs.plan(21, N_CU)[2] == [3, 4, 3, 4, 3, 4]


def test_the_other_sweeps_and_the_batch_reach_their_shapes():
    assert {gs.plan(F, N_CU)[0] for F in gs.SWEEP_STEP} == {"tiny", "p4", "p8", "launch"}
    assert {gs.shape_class(F, N_CU) for F in gs.SWEEP_STEP} >= {"p4-all4", "p4-3-inside", "p4-3-first-only", "p8-tf5-mixed", "p8-tf8-mixed"}
    assert all(F >= gs.TINY_BELOW for F in gs.SWEEP_LAUNCH)  # XDTTS_GL=launch: k_gl_fused, last block of 1, 3 or 4 frames
    assert {F % 4 for F in gs.SWEEP_LAUNCH} >= {0, 1, 2, 3}
    assert [gs.shape_class(F, N_CU) for F in gs.SWEEP_SEEDED] == ["p4-3-inside", "p8-tf5-mixed"]
    own4, own8 = set(), set()
    for F in gs.BATCH_FRAMES:
        s4, s8 = gs.batch_split(F, 4, N_CU), gs.batch_split(F, 8, N_CU)
        if F < gs.TINY_BELOW:
            assert s4 is None and s8 is None
            continue
        assert sum(s4) == sum(s8) == F and s4 == gs.plan(F, N_CU)[2]
        own4 |= set(s4)
        own8 |= set(s8)
    assert own4 == {3, 4} and own8 == {5, 6, 7, 8}  # own frames 3 .. 8 over the two batch shapes
    assert sum(len(gs.batch_split(F, 4, N_CU) or []) for F in gs.BATCH_FRAMES) <= N_CU  # one launch, so the offsets are exercised together


def test_the_hop_metric_sees_one_spoilt_boundary_at_full_size():
    """768 wrong samples of size 0.05 at one boundary: the whole-signal RMS shrinks with the utterance's length,
    the worst hop does not."""
    for F in (17, 2049):
        ref = gs.chirps(gs.HOP * (F - 1))
        a = ref.copy()
        b0 = gs.HOP * (F // 2)
        a[b0:b0 + 3 * gs.HOP] += 0.05
        assert abs(gs.worst_hop(a, ref) - 0.05) < 1e-6
        assert abs(gs.rms(a, ref) - 0.05 * np.sqrt(3.0 / (F - 1))) < 1e-6
        h = gs.hop_rms(a, ref)
        assert h.shape == (F - 1,) and int((h > 0).sum()) == 3
    with pytest.raises(AssertionError):
        gs.worst_hop(np.zeros(100), np.zeros(100))


def test_per_frame_rel_sees_one_misplaced_row():
    rng = np.random.default_rng(0)
    ref = rng.standard_normal((gs.N_BINS, 40, 2))
    r = ref.copy()
    r[:, 7] = ref[:, 8]  # one frame's row taken from its neighbour
    e = gs.per_frame_rel(r, ref)
    assert e.shape == (40,) and e[7] > 1.0 and np.all(np.delete(e, 7) == 0.0)
    assert gs.rms(r, ref) / float(np.sqrt(np.mean(ref ** 2))) < 0.25  # the overall figure already dilutes it at 40 frames
